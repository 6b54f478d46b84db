// ---------------------------------------------------------------- fp32 conv on bf16 MFMAs (3-plane split)
// The fp32 Conv3d 160 -> 160 (forward / dgrad) computed with bf16 matrix cores
// to fp32 accuracy.  Every fp32 operand is split into three bf16 planes,
//   x = xh + xm + xl,  xh = bf16(x), xm = bf16(x - xh), xl = bf16(x - xh - xm)
// (each residual exact in fp32, 8 more significant bits per plane: 24 bits in
// all), and the product is the six plane products whose weight is >= 2^-16:
//   x w ~ xh wh + xh wm + xm wh + xh wl + xl wh + xm wm
// (dropped: xm wl, xl wm, xl wl <= 2^-24 relative).  Each bf16 product is exact
// in the fp32 MFMA accumulator, so the result is an fp32 GEMM with a different
// summation order: on the Conv3d 160 -> 160 its NRMSE vs float64 is 1.5e-7
// against 3.6e-7 for PyTorch's fp32 conv (tools/x6_numerics.py).
//
// Six bf16 MFMAs cost 6 x 16 = 96 cycles per 16x16x32 block against 8 x 32 =
// 256 for the f32 MFMA (v_mfma_f32_16x16x4_f32) -- 2.67x fewer matrix-core
// cycles for the same fp32-accurate result.
//
// Operands: activations as XA [rows][320] bf16 (per 16-channel chunk c: xh then
// xm, 64 B at 64 c) and XB [rows][160] (xl, 32 B at 32 c) -- dlcs_split3_bf16;
// weights as WA [27][160][320] (wh | wm per chunk) and WB [27][160][160] (wl)
// -- dlcs_conv3d_pack_weights modes 2 / 3.  Over one 16-channel chunk the six
// products are three v_mfma_f32_16x16x32_bf16 (k = 32 = two 16-channel plane
// segments; lane group cq supplies k = 8 cq .. 8 cq + 7):
//   P1: A = [xh | xh], B = [wh | wm]     (xh wh + xh wm)
//   P2: A = [xm | xl], B = [wh | wh]     (xm wh + xl wh)
//   P3: A = [xh | xm], B = [wl | wm]     (xh wl + xm wm)
// Tile, waves and epilogue are the fp32 kernel's (256 voxels x 160 channels,
// 8 waves x 4 x 5 tiles of 16x16); per step (one 16-channel chunk x 3 kw taps)
// a wave issues 180 MFMAs.  LDS: the chunk's halo images X1 [600][32] (xh | xm,
// 64-B rows, the v5 swizzle) and X2 [600][16] (xl, 32-B rows, 16-B halves
// swapped by bit 1 of halo y: the fewest ds_read_b128 conflicts of any swizzle
// on (y, x) mod 4, tools/x6_swizzle.py) single-buffered (the next chunk waits in registers
// and is stored behind an extra barrier at the seam), weight slices W1
// [3][160][32] and W2 [3][160][16] double-buffered by DMA: 146 KB.

constexpr int kX6H1 = kHalo * 32;              // bf16 in X1 (38.4 KB)
constexpr int kX6H2 = kHalo * 16;              // bf16 in X2 (19.2 KB)
constexpr int kX6W1 = 3 * 160 * 32;            // bf16 in a W1 slice (30 KB)
constexpr int kX6W2 = 3 * 160 * 16;            // bf16 in a W2 slice (15 KB)
constexpr int kX6Slot = kX6W1 + kX6W2;

struct ConvX6Args {
    const bf16* xa; const bf16* xb; const bf16* w;   // w: WA then WB
    const float* bias; float* out; const float* mask; const float* res;
    int B, D, H, W;
    int cout_ld, mask_ld, res_ld, accumulate, relu_out;
    float res_scale;
};

template <int EPI>
__global__ void __launch_bounds__(512) conv3d_k3_x6_kernel(ConvX6Args a) {
    constexpr int CO = 160;
    __shared__ __attribute__((aligned(16))) bf16 smem_x6[kX6H1 + kX6H2 + 2 * kX6Slot];   // 146.25 KB
    bf16* X1 = smem_x6;
    bf16* X2 = X1 + kX6H1;
    bf16* Ws = X2 + kX6H2;

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
    constexpr int NCC = 10;                            // 16-channel chunks
    constexpr int NSTEPS = NCC * 9;                    // step s: chunk s / 9, tap row s % 9

    // halo pieces of this thread: X1 2400 16-B pieces (5 per thread), X2 1200 (3)
    constexpr int P1 = 5, P2 = 3;
    bf16x8_t hr[P1 + P2];
    int hoff[P1 + P2];
#pragma unroll
    for (int k = 0; k < P1 + P2; ++k) {
        const bool x1 = k < P1;
        const int i = threadIdx.x + (x1 ? k : k - P1) * 512;
        const int npc = x1 ? 4 : 2;                    // pieces per halo row
        hoff[k] = -1;
        if (i < kHalo * npc) {
            const int hv = i / npc, c = i % npc;
            const int ht = hv / (kHaloY * kHaloX), hy = (hv / kHaloX) % kHaloY, hx = hv % kHaloX;
            const int t = t0 - 1 + ht, y = y0 - 1 + hy, x = x0 - 1 + hx;
            if (t >= 0 && t < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W)
                hoff[k] = (int)(brow(b, t, y, x, nT, nY, nX) * (x1 ? 320 : 160) + c * 8);
        }
    }
    auto load_halo = [&](int cc) {
#pragma unroll
        for (int k = 0; k < P1 + P2; ++k) {
            const bf16* base = k < P1 ? a.xa + cc * 32 : a.xb + cc * 16;
            hr[k] = (bf16x8_t)(bf16)0.0f;
            if (hoff[k] >= 0) hr[k] = *reinterpret_cast<const bf16x8_t*>(base + hoff[k]);
        }
    };
    auto store_halo = [&]() {
#pragma unroll
        for (int k = 0; k < P1 + P2; ++k) {
            const bool x1 = k < P1;
            const int i = threadIdx.x + (x1 ? k : k - P1) * 512;
            const int npc = x1 ? 4 : 2;
            if (i < kHalo * npc) {
                const int hv = i / npc, c = i % npc;
                const int hy = (hv / kHaloX) % kHaloY;
                if (x1) *reinterpret_cast<bf16x8_t*>(X1 + hv * 32 + ((c ^ ((hy & 1) << 1)) << 3)) = hr[k];
                else    *reinterpret_cast<bf16x8_t*>(X2 + hv * 16 + ((c ^ ((hy >> 1) & 1)) << 3)) = hr[k];
            }
        }
    };
    // weight DMA of step s into slot s & 1: W1 30 pieces (64-B rows, v5 swizzle),
    // W2 15 pieces (32-B rows, unswizzled: the b128 lane groups of a read already
    // hit 16 distinct 16-B bank quads); piece wi by wave wi % 8
    const unsigned wbase = lds_offset(Ws);
    unsigned woff[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int wi = k * 8 + wave;
        woff[k] = 0;
        if (wi < 30) {
            const int c = wi * 64 + lane;
            const int row = c >> 2, pos = c & 3;
            const int tl = row / CO, co = row % CO;
            const int kl = pos ^ ((4 - ((co & 15) >> 2)) & 3);
            woff[k] = (unsigned)(((tl * CO + co) * 320 + (kl << 3)) * 2);
        } else if (wi < 45) {
            const int c = (wi - 30) * 64 + lane;
            const int row = c >> 1, pos = c & 1;
            const int tl = row / CO, co = row % CO;
            woff[k] = (unsigned)(((tl * CO + co) * 160 + (pos << 3)) * 2);
        }
    }
    const bf16* wa = a.w;
    const bf16* wb = a.w + 27L * CO * 320;
    auto issue_w = [&](int s) {
        const int cc = s / 9, t3 = (s % 9) * 3;
        const unsigned dst = wbase + (unsigned)((s & 1) * kX6Slot * 2);
        const bf16* s1 = wa + (long)t3 * CO * 320 + cc * 32;
        const bf16* s2 = wb + (long)t3 * CO * 160 + cc * 16;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int wi = k * 8 + wave;
            if (wi < 30) glds16_s(s1, woff[k], dst + wi * 1024);
            else if (wi < 45) glds16_s(s2, woff[k], dst + kX6W1 * 2 + (wi - 30) * 1024);
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
    const int bsw = (4 - (vq >> 2)) & 3;               // W1 chunk swizzle of this lane's co rows (co & 15 = vq)

    // A / B fragment addresses of pack p for lane group cq (see the header)
    auto read_frags = [&](int s, int kw, int p, bf16x8_t (&af)[4], bf16x8_t (&bfr)[5]) {
        const int st = s % 9, kd = st / 3, kh = st % 3;
        const int hp = (ly + kh) & 1;
        const int toff = (kd * kHaloY + kh) * kHaloX + kw;
        // A: image, row length, element offset inside the row
        const bf16* img;
        int ald, aoff;
        if (p == 0) { img = X1; ald = 32; aoff = ((cq & 1) ^ (hp << 1)) << 3; }
        else if (p == 1) {
            if (cq < 2) { img = X1; ald = 32; aoff = ((2 + cq) ^ (hp << 1)) << 3; }
            else        { img = X2; ald = 16; aoff = ((cq - 2) ^ (((ly + kh) >> 1) & 1)) << 3; }
        } else { img = X1; ald = 32; aoff = (cq ^ (hp << 1)) << 3; }
        const bf16* wsl = Ws + (s & 1) * kX6Slot;
        const bf16* wimg;
        int bld, boff;
        if (p == 0) { wimg = wsl; bld = 32; boff = (cq ^ bsw) << 3; }
        else if (p == 1) { wimg = wsl; bld = 32; boff = ((cq & 1) ^ bsw) << 3; }
        else {
            if (cq < 2) { wimg = wsl + kX6W1; bld = 16; boff = cq << 3; }
            else        { wimg = wsl; bld = 32; boff = (cq ^ bsw) << 3; }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            af[i] = *reinterpret_cast<const bf16x8_t*>(img + (hb0 + i * kHaloY * kHaloX + toff) * ald + aoff);
#pragma unroll
        for (int j = 0; j < 5; ++j)
            bfr[j] = *reinterpret_cast<const bf16x8_t*>(wimg + (kw * CO + corow + j * 16) * bld + boff);
    };
    auto mma = [&](const bf16x8_t (&af)[4], const bf16x8_t (&bfr)[5]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) mfma16(acc[i][j], af[i], bfr[j]);
    };

    load_halo(0);
    issue_w(0);
    store_halo();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
    for (int s = 0; s < NSTEPS; ++s) {
        const int sc = s % 9;
        const bool seam = (sc == 8) && (s + 1 < NSTEPS);
        if (sc == 7 && s + 2 < NSTEPS) load_halo(s / 9 + 1);
        const bool dma = s + 1 < NSTEPS;
        bf16x8_t afA[4], bfA[5], afB[4], bfB[5];
        if (dma && wave < 4) issue_w(s + 1);
        // 9 units (kw, pack), two fragment sets in flight
        read_frags(s, 0, 0, afA, bfA);
#pragma unroll
        for (int u = 0; u < 9; u += 2) {
            if (u + 1 < 9) read_frags(s, (u + 1) / 3, (u + 1) % 3, afB, bfB);
            mma(afA, bfA);
            if (u == 0 && dma && wave >= 4) issue_w(s + 1);
            if (u + 2 < 9) read_frags(s, (u + 2) / 3, (u + 2) % 3, afA, bfA);
            if (u + 1 < 9) mma(afB, bfB);
        }
        if (seam) {
            __syncthreads();                           // every wave is done with this chunk's halo
            store_halo();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // step s+1's weight slice has landed
        __syncthreads();
    }
    ConvF32Args ea{};
    ea.bias = a.bias; ea.out = a.out; ea.mask = a.mask; ea.res = a.res;
    ea.cout_ld = a.cout_ld; ea.mask_ld = a.mask_ld; ea.res_ld = a.res_ld; ea.accumulate = a.accumulate;
    ea.relu_out = a.relu_out; ea.res_scale = a.res_scale;
    conv_epilogue_f32<EPI>(ea, acc, reinterpret_cast<float*>(smem_x6), pw, nh * 80, lane, b, pt, tyy * 2, txx * 2,
                           nT, nY, nX);
}

// x [rows][ld] fp32 (160 channels) -> XA [rows][320] (xh | xm per 16-channel
// chunk), XB [rows][160] (xl); one thread per 8 channels of a row
__global__ void split3_kernel(const float* x, long rows, int ld, bf16* xa, bf16* xb) {
    const long n = rows * 20;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / 20;
        const int c8 = (int)(i % 20) * 8;              // first channel
        const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(x + r * ld + c8);
        const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(x + r * ld + c8 + 4);
        bf16x8_t h, m, l;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = e < 4 ? v0[e] : v1[e - 4];
            const bf16 hv = (bf16)v;
            const float r1 = v - (float)hv;
            const bf16 mv = (bf16)r1;
            const float r2 = r1 - (float)mv;
            h[e] = hv; m[e] = mv; l[e] = (bf16)r2;
        }
        const int cc = c8 >> 4, half = (c8 >> 3) & 1;
        *reinterpret_cast<bf16x8_t*>(xa + r * 320 + cc * 32 + half * 8) = h;
        *reinterpret_cast<bf16x8_t*>(xa + r * 320 + cc * 32 + 16 + half * 8) = m;
        *reinterpret_cast<bf16x8_t*>(xb + r * 160 + c8) = l;
    }
}

// weights [160][160][27] fp32 -> WA [27][160][320] (wh | wm per 16-channel
// chunk of the contracted index), WB [27][160][160] (wl);
// mode 0: rows co, contracted ci, tap t;  mode 1 (dgrad): rows ci, contracted co, tap 26 - t
__global__ void pack_weights_x6_kernel(const float* w, bf16* wa, bf16* wb, int mode) {
    const long n = 27L * 160 * 160;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % 160);
        const int r = (int)((i / 160) % 160);
        const int tap = (int)(i / (160L * 160));
        const float v = mode == 0 ? w[((long)r * 160 + c) * 27 + tap] : w[((long)c * 160 + r) * 27 + (26 - tap)];
        const bf16 hv = (bf16)v;
        const float r1 = v - (float)hv;
        const bf16 mv = (bf16)r1;
        const float r2 = r1 - (float)mv;
        const long row = (long)tap * 160 + r;
        wa[row * 320 + (c >> 4) * 32 + (c & 15)] = hv;
        wa[row * 320 + (c >> 4) * 32 + 16 + (c & 15)] = mv;
        wb[row * 160 + c] = (bf16)r2;
    }
}

static int conv_x6_launch(const ConvX6Args& v, hipStream_t st) {
    const unsigned nblk = (unsigned)conv_tiles(v.B, v.D, v.H, v.W);
    const int epi = conv_epi_code(v.res, v.mask, !v.accumulate, true);
    if (epi == 0) hipLaunchKernelGGL(conv3d_k3_x6_kernel<0>, dim3(nblk), dim3(512), 0, st, v);
    else if (epi == kEpiRes) hipLaunchKernelGGL(conv3d_k3_x6_kernel<kEpiRes>, dim3(nblk), dim3(512), 0, st, v);
    else if (epi == kEpiMask) hipLaunchKernelGGL(conv3d_k3_x6_kernel<kEpiMask>, dim3(nblk), dim3(512), 0, st, v);
    else hipLaunchKernelGGL(conv3d_k3_x6_kernel<kEpiGeneric>, dim3(nblk), dim3(512), 0, st, v);
    return dlcs_launch_status();
}

// ---------------------------------------------------------------- wgrad on bf16 matrix cores (3-plane split)
// dW[tap][co][ci] = sum_v g[v][co] x[v + off(tap)][ci] with g and x split into
// bf16 planes (dlcs_split3_bf16 layout) and the six plane products >= 2^-16;
// K = voxels.  Over 16 voxels the six products are three 16x16x32 MFMAs (lane
// group gq supplies k = 8 gq .. 8 gq + 7 = voxels 8 (gq & 1) .. + 7 of one
// plane; groups 0-1 and 2-3 carry the two plane segments of a pack):
//   P1: A = [gh | gh], B = [xh | xm]   P2: A = [gm | gl], B = [xh | xh]
//   P3: A = [gh | gm], B = [xl | xm]
// Work split of conv3d_wgrad_f32_kernel / conv3d_wgrad_c160_kernel: workgroup =
// tap row (kd, kh) x voxel range, 12 waves = 3 kw taps x 2 co halves x 2 ci
// halves (80 x 80 of dW[tap] each, 5 x 5 tiles).  Unit = half patch (32 voxels):
// per plane its g rows [32][160] and the tap row's x halo [2 t][4 y][6 x][160],
// 76.8 KB for the three planes, DMA'd global -> LDS one unit ahead into two
// buffers; operands read voxel-contiguous with ds_read_b64_tr_b16 (16-channel
// tiles XOR-swizzled by bit 1 of the 8-voxel group, as the bf16 kernel).
constexpr int kWxRows = 32 + 48;
constexpr int kWxPlane = kWxRows * 160;              // bf16 per plane image (25.6 KB)
constexpr int kWxBuf = 3 * kWxPlane;                 // 76.8 KB

struct WgradX6Args {
    const bf16* ga; const bf16* gb;                  // g planes (320 / 160 columns)
    const bf16* xa; const bf16* xb;                  // x planes
    float* dw;
    int B, D, H, W;
};

__global__ void __launch_bounds__(768) conv3d_wgrad_x6_kernel(WgradX6Args a, int nrange, long ppr, int xcd_map) {
    __shared__ __attribute__((aligned(16))) bf16 smem_wx[2 * kWxBuf];     // 153.6 KB
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
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kwi = wave >> 2, coh = (wave >> 1) & 1, cih = wave & 1;
    const bf16* zrow = reinterpret_cast<const bf16*>(g_wg_zero_row);

    // DMA of unit u: 75 wave-instructions; instruction wi: plane wi / 25, rows
    // 0..31 (g, instructions 0..9 of a plane) or 32..79 (halo, 10..24).  Chunk
    // kp of a row holds the logical 8-channel chunk kp ^ (2 swz).
    auto issue = [&](long u, int buf) {
        const long patch = u >> 1;
        const int th = (int)(u & 1);
        const int px = (int)(patch % nX);
        long r = patch / nX;
        const int py = (int)(r % nY); r /= nY;
        const int pt = (int)(r % nT);
        const int bb = (int)(r / nT);
        const unsigned dst = __builtin_amdgcn_readfirstlane(lds_offset(smem_wx) + buf * kWxBuf * 2);
        int ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll 1
        for (int k = 0; k < 7; ++k) {
            const int wi = k * 12 + wave;
            if (wi >= 75) break;
            const int pl = wi / 25, wl = wi - pl * 25;
            const int c = wl * 64 + ln;
            const int row = c / 20, kp = c - row * 20;
            long vrow;
            bool ok = true;
            int swz;
            if (wl < 10) {
                vrow = patch * 64 + th * 32 + row;
                swz = (row >> 3) & 1;
            } else {
                const int hr = row - 32, ty = hr / 6, xh = hr - ty * 6;
                const int tl = ty >> 2, y = ty & 3;
                swz = (y >> 1) & 1;
                const int T = pt * 4 + th * 2 + tl + kd, Y = py * 4 + y + kh, X = px * 4 + xh - 1;
                ok = (unsigned)T < (unsigned)a.D && (unsigned)Y < (unsigned)a.H && (unsigned)X < (unsigned)a.W;
                vrow = ((((long)(bb * nT + (T >> 2)) * nY + (Y >> 2)) * nX + (X >> 2)) << 6) + ((T & 3) << 4) +
                       ((Y & 3) << 2) + (X & 3);
            }
            const int kl = kp ^ (swz << 1);
            const bf16* pa = wl < 10 ? a.ga : a.xa;
            const bf16* pb = wl < 10 ? a.gb : a.xb;
            const bf16* src;
            if (pl == 2) src = pb + vrow * 160 + 8 * kl;
            else src = pa + vrow * 320 + 32 * (kl >> 1) + 16 * pl + 8 * (kl & 1);
            glds16(ok ? src : zrow, dst + (pl * kWxPlane) * 2 + wl * 1024);
        }
    };

    f32x4_t acc[5][5];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[i][j] = (f32x4_t)0.0f;

    const int gq = lane >> 4, q = (lane >> 2) & 3, p4 = (lane & 3) * 4, swb = gq & 1;
    // planes of the three packs for this lane group (header)
    const int pA0 = 0, pB0 = gq < 2 ? 0 : 1;
    const int pA1 = gq < 2 ? 1 : 2, pB1 = 0;
    const int pA2 = gq < 2 ? 0 : 1, pB2 = gq < 2 ? 2 : 1;
    auto acol = [&](int i) { return (((coh * 5 + i) ^ swb) << 4) + p4; };
    auto bcol = [&](int j) { return (((cih * 5 + j) ^ swb) << 4) + p4; };

    const long u0 = 2 * p0, u1 = 2 * p1;
    issue(u0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (long u = u0; u < u1; ++u) {
        if (u + 1 < u1) issue(u + 1, cur ^ 1);
        const bf16* S = smem_wx + cur * kWxBuf;
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int grow = (16 * h + 8 * swb + q) * 160;
            const int xrow = (32 + (4 * h + 2 * swb) * 6 + q + kwi) * 160;
#pragma unroll
            for (int pk = 0; pk < 3; ++pk) {
                const int pA = pk == 0 ? pA0 : (pk == 1 ? pA1 : pA2);
                const int pB = pk == 0 ? pB0 : (pk == 1 ? pB1 : pB2);
                const bf16* Gb = S + pA * kWxPlane + grow;
                const bf16* Xb = S + pB * kWxPlane + xrow;
                bf16x8_t af[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) af[i] = tr_read16(Gb + acol(i), Gb + 4 * 160 + acol(i));
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const bf16x8_t bfr = tr_read16(Xb + bcol(j), Xb + 6 * 160 + bcol(j));
#pragma unroll
                    for (int i = 0; i < 5; ++i) mfma16(acc[i][j], af[i], bfr);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }
    const int tap = (kd + 1) * 9 + (kh + 1) * 3 + kwi;
    float* dw = a.dw + (long)tap * 160 * 160;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = coh * 80 + 16 * i + gq * 4 + r, ci = cih * 80 + 16 * j + (lane & 15);
                atomicAdd(dw + co * 160 + ci, acc[i][j][r]);
            }
}

static int wgrad_x6_launch(const WgradX6Args& a, hipStream_t st) {
    const long npatch = (long)a.B * (a.D / 4) * (a.H / 4) * (a.W / 4);
    static const int env_nr = [] { const char* e = dlcs_knob("DLCS_WGX6_RANGES"); return e ? atoi(e) : 0; }();
    int nr = env_nr > 0 ? env_nr : 28;
    nr = (int)std::min<long>(nr, npatch);
    const long pp = (npatch + nr - 1) / nr;
    nr = (int)((npatch + pp - 1) / pp);
    const int xcd_map = (nr % 8 == 0) ? 1 : 0;
    hipLaunchKernelGGL(conv3d_wgrad_x6_kernel, dim3((unsigned)(9 * nr)), dim3(768), 0, st, a, nr, pp, xcd_map);
    return dlcs_launch_status();
}
