// ---------------------------------------------------------------- fp32 token Linears on fp16 matrix cores, row-scaled split (h3r)
// Included by gemm_f16x3.hip (mfma16h, f16x3_scale: f16x3_common.h; glds16: lds_dma.h).
//
// C[row(m), n] (+)= alpha act(sum_k A[m, k] B[n, k] + bias[n]) + res[row(m), n]
// for the fp32 token Linears: the Swin block's (vst:146, :168, :33-37; K in
// {160, 480, 640}, N a multiple of 160) and the DiT / Latte blocks' (dit:317-350,
// lat:301-316 and the DiT / Latte patch GEMMs; K a multiple of 64 in segments of
// 192 / 128 / 64, N of 64), forwards and input gradients.
//
// The split of conv3d_f16x3.inc (u = s x, xh = f16(u), xl = f16(u - xh), three
// plane products hh + hl + lh), but with one power-of-two scale PER ROW of each
// operand instead of one per tensor:
//   * A (the fp32 activation) is read as fp32 straight from HBM: every thread
//     holds its row's share of one K segment (NCH chunks of 32) in registers, the
//     row max comes from three lane shuffles, and the split is written into a
//     2-slot LDS ring chunk by chunk -- no max-abs pass, no memset, no split
//     launch, no planes in HBM.  K longer than one segment (DiT: K = 1152, 1536)
//     runs as nseg segments, each with its own row scale: the segment's partial
//     tile is folded into an fp32 total with 1 / s_a[m, seg] (exact) and the next
//     segment's rows are loaded during the current one (each chunk register is
//     reloaded as soon as its split is written);
//   * B (the weight, or its transpose for an input gradient) is packed by
//     dlcs_h3r_pack_multi: planes [N][K / 32][xh 32 | xl 32] plus 1 / s per row;
//   * the tile is rescaled by (1 / s_b[n]) in the epilogue (exact).
// A row scale adapts to each token's own magnitude, so the dynamic-range limit
// of a per-tensor scale (elements 2^17 below the tensor max lose their low
// plane) moves to 2^17 below the ROW (segment) max.
//
// Tile 64 x 32 NJ (NJ = 5: 160, 4: 128, 2: 64), 8 waves of 16 x 16 NJ
// (v_mfma_f32_16x16x32_f16, K = 32 of one plane), A ring 2 x 8 KB, B ring
// 3 x 4 NJ KB DMA'd two chunks ahead (NJ = 5: 76 KB, two workgroups per CU).
// Tiles are numbered XCD-major with n fastest, so the N / 32 NJ tiles sharing an
// A row block run on one XCD and read it through one L2.
struct GemmH3rArgs {
    const float* a; long lda; int M;
    const f16* bp; const float* binv; int N;
    float* c; long ldc;
    const float* bias; int act; float alpha;
    const float* res; long ldr;
    const int* row_map;
    int accumulate;
    const float* aux; float* aux_out; long ldaux;
    int ntn, ntiles, per_xcd;
    int nseg;                                         // K = nseg * NCH * 32
    int ksplit;                                       // 1, or K ranges 2 / 4 / 8 (part != null)
    float* part;                                      // [ksplit][M][N] raw partial tiles (split K)
};
constexpr int kHrA = 64 * 64;                         // f16 per A chunk slot (8 KB)

// s_waitcnt vmcnt(n) for a wave-uniform n in 0..4
DLCS_DEV void hr_vmwait(int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    }
}

template <int NCH, int NJ, bool SEG>
__global__ void __launch_bounds__(512, 2) gemm_h3r_kernel(GemmH3rArgs g) {
    constexpr int NT = 32 * NJ, KB = NT * 64;         // N tile; f16 per B chunk slot
    __shared__ __attribute__((aligned(16))) f16 smem_hr[2 * kHrA + 3 * KB];
    __shared__ float ainv_s[2][64];
    const int b = blockIdx.x;
    // split K: K range kp = XCD % ksplit, so an XCD streams 1 / ksplit of B (its L2 holds it)
    const int xcd = b & 7, ngrp = 8 / g.ksplit;
    const int kp = xcd % g.ksplit;
    const int tile = (xcd / g.ksplit) * g.per_xcd + (b >> 3);
    if (tile >= g.ntiles) return;                     // no barrier has run yet
    const int m0 = (tile / g.ntn) * 64, n0 = (tile % g.ntn) * NT;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave & 3, wn = wave >> 2;
    const unsigned sbase = lds_offset(smem_hr);
    const int nsegt = SEG ? g.nseg : 1;               // segments of the whole K
    const int sg0 = SEG ? (int)((long)nsegt * kp / g.ksplit) : 0;
    const int nseg = SEG ? (int)((long)nsegt * (kp + 1) / g.ksplit) - sg0 : 1;
    const int ncht = nseg * NCH;                      // chunks of 32 over this K range
    const long BLD = (long)nsegt * NCH * 64;          // f16 per packed B row (the whole K)
    (void)ngrp;

    // A: thread (row ar, quarter aj) holds columns 32 c + 4 aj .. + 3 of every chunk c of a segment
    const int ar = threadIdx.x >> 3, aj = threadIdx.x & 7;
    const float* arow = g.a + (long)min(m0 + ar, g.M - 1) * g.lda + (long)sg0 * NCH * 32 + 4 * aj;
    f32x4_t xa[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) xa[c] = *reinterpret_cast<const f32x4_t*>(arow + 32 * c);

    // B chunk cc -> slot: 4 NJ DMA instructions of 8 rows, round-robin over the waves
    auto issue_b = [&](int cc, int slot) {
        for (int rb = wave; rb < 4 * NJ; rb += 8) {
            const int r = rb * 8 + (lane >> 3), pc = lane & 7;
            const int lc = pc ^ ((r >> 1) & 7);
            const f16* src = g.bp + (long)(n0 + r) * BLD + ((long)sg0 * NCH + cc) * 64 + lc * 8;
            glds16(src, sbase + (unsigned)((2 * kHrA + slot * KB) * 2 + rb * 1024));
        }
    };
    const int nb = (4 * NJ - wave + 7) / 8;           // this wave's DMA instructions per B chunk
    issue_b(0, 0);
    if (ncht > 1) issue_b(1, 1);

    // row max over the segment held in xa: the 8 threads of a row are 8 consecutive lanes
    auto row_scale = [&]() {
        float mx = 0.0f;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(xa[c][0]), fabsf(xa[c][1])), fmaxf(fabsf(xa[c][2]), fabsf(xa[c][3]))));
        return f16x3_scale(__float_as_uint(lane8_max(mx)));
    };
    // odd rows take a negative scale: their planes, tiles and sums are negated and the
    // epilogue's 1 / s restores the sign, so the matrix core's truncation toward -inf
    // (a sign-independent bias, tools/probe/mfma_chain.hip) alternates between
    // neighbouring rows and cancels in any later sum over rows (bias / norm gradients)
    const float rsg = ((m0 + ar) & 1) ? -1.0f : 1.0f;
    float sa = rsg * row_scale();
    if (aj == 0) ainv_s[0][ar] = 1.0f / sa;
    // split of a chunk into an A slot: xh in 16-B piece aj / 2, xl in piece 4 + aj / 2
    // (pieces XOR-swizzled by (row / 2) & 7, the conv kernels' 128-B-row pattern)
    const int asw = (ar >> 1) & 7;
    const int aoh = ar * 64 + (((aj >> 1) ^ asw) << 3) + (aj & 1) * 4;
    const int aol = ar * 64 + (((4 + (aj >> 1)) ^ asw) << 3) + (aj & 1) * 4;
    auto split_a = [&](const f32x4_t& v, int slot) {
        f16x4_t h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float u = v[e] * sa;
            const f16 hv = (f16)u;
            h[e] = hv;
            l[e] = (f16)(u - (float)hv);
        }
        *reinterpret_cast<f16x4_t*>(smem_hr + slot * kHrA + aoh) = h;
        *reinterpret_cast<f16x4_t*>(smem_hr + slot * kHrA + aol) = l;
    };
    split_a(xa[0], 0);

    f32x4_t acc[NJ], tot[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = tot[j] = (f32x4_t)0.0f;
    const int vq = lane & 15, cq = lane >> 4, sw = (vq >> 1) & 7;
    const int oh = (cq ^ sw) << 3, ol = ((4 + cq) ^ sw) << 3;
    hr_vmwait(ncht > 1 ? nb : 0);
    __syncthreads();
    for (int seg = 0; seg < nseg; ++seg) {
        const bool more = SEG && seg + 1 < nseg;
        const float* nrow = arow + (long)(seg + 1) * NCH * 32;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int cc = seg * NCH + c;
            int na = 0;                               // A loads issued in this chunk (next segment)
            if (c + 1 < NCH) split_a(xa[c + 1], (cc + 1) & 1);
            if (cc + 2 < ncht) issue_b(cc + 2, (cc + 2) % 3);
            if (more) {                               // xa[c + 1] (and at c = 0 xa[0]) are dead: reload
                if (c == 0) { xa[0] = *reinterpret_cast<const f32x4_t*>(nrow); ++na; }
                if (c + 1 < NCH) { xa[c + 1] = *reinterpret_cast<const f32x4_t*>(nrow + 32 * (c + 1)); ++na; }
            }
            const f16* As = smem_hr + (cc & 1) * kHrA + (wm * 16 + vq) * 64;
            const f16* Bs = smem_hr + 2 * kHrA + (cc % 3) * KB + (wn * 16 * NJ + vq) * 64;
            const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(As + oh);
            const f16x8_t al = *reinterpret_cast<const f16x8_t*>(As + ol);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f16x8_t bh = *reinterpret_cast<const f16x8_t*>(Bs + j * 16 * 64 + oh);
                const f16x8_t bl = *reinterpret_cast<const f16x8_t*>(Bs + j * 16 * 64 + ol);
                mfma16h(acc[j], ah, bh);
                mfma16h(acc[j], ah, bl);
                mfma16h(acc[j], al, bh);
            }
            if (c == NCH - 1) {
                // fold the segment's tile with its row scales (rows wm 16 + 4 cq + r)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float ia = ainv_s[seg & 1][wm * 16 + 4 * cq + r];
#pragma unroll
                    for (int j = 0; j < NJ; ++j) tot[j][r] += acc[j][r] * ia;
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] = (f32x4_t)0.0f;
                if (more) {                           // the next segment's scale and first chunk
                    sa = rsg * row_scale();
                    if (aj == 0) ainv_s[(seg + 1) & 1][ar] = 1.0f / sa;
                    split_a(xa[0], (cc + 1) & 1);
                }
            }
            hr_vmwait(cc + 2 < ncht ? nb + na : na);
            __syncthreads();
        }
    }
    // epilogue, staged through LDS (operand images dead after the last barrier)
    float* Es = reinterpret_cast<float*>(smem_hr);       // [64][NT + 4]
    constexpr int EL = NT + 4;
    float binv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) binv[j] = g.binv[n0 + wn * 16 * NJ + j * 16 + vq];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = wm * 16 + 4 * cq + r;
#pragma unroll
        for (int j = 0; j < NJ; ++j) Es[row * EL + wn * 16 * NJ + j * 16 + vq] = tot[j][r] * binv[j];
    }
    __syncthreads();
    constexpr int PR = NT / 4;                            // 16-B pieces per row
    if (g.part) {                                         // split K: the raw partial tile
        float* pp = g.part + (long)kp * g.M * g.N;
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int q = threadIdx.x + k * 512;
            const int ml = q / PR, ch = (q % PR) * 4;
            const long m = m0 + ml, n = n0 + ch;
            if (m < g.M) *reinterpret_cast<f32x4_t*>(pp + m * g.N + n) = *reinterpret_cast<const f32x4_t*>(Es + ml * EL + ch);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
        const int q = threadIdx.x + k * 512;              // 64 rows x PR pieces
        const int ml = q / PR, ch = (q % PR) * 4;
        const long m = m0 + ml, n = n0 + ch;
        if (m >= g.M) continue;
        long orow = m;
        if (g.row_map) {
            orow = g.row_map[m];
            if (orow < 0) continue;
        }
        f32x4_t v = *reinterpret_cast<const f32x4_t*>(Es + ml * EL + ch);
        if (g.bias) v += *reinterpret_cast<const f32x4_t*>(g.bias + n);
        if (act_is_fwd(g.act)) {
            if (g.aux_out && g.act != 3) *reinterpret_cast<f32x4_t*>(g.aux_out + m * g.ldaux + n) = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = act_fwd(g.act, v[e]);
        } else if (act_is_grad(g.act)) {
            const f32x4_t av = *reinterpret_cast<const f32x4_t*>(g.aux + m * g.ldaux + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= act_grad_scale(g.act, av[e]);
        }
        v *= g.alpha;
        if (g.res) v += *reinterpret_cast<const f32x4_t*>(g.res + orow * g.ldr + n);
        if (g.act == 7) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
        }
        float* cp = g.c + orow * g.ldc + n;
        if (g.accumulate) v += *reinterpret_cast<const f32x4_t*>(cp);
        *reinterpret_cast<f32x4_t*>(cp) = v;
    }
}

// split-K h3r: C[m, n] (+)= alpha (sum_kp part[kp][m][n] + bias[n]) + res[m, n], the K
// ranges summed in a fixed order (run-to-run deterministic); act = 0, no row map
__global__ void __launch_bounds__(256) h3r_ksplit_reduce_kernel(GemmH3rArgs g) {
    const long nq = (long)g.M * g.N / 4;
    const long sl = (long)g.M * g.N;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const long m = q * 4 / g.N, n = q * 4 % g.N;
        f32x4_t v = *reinterpret_cast<const f32x4_t*>(g.part + q * 4);
        for (int k = 1; k < g.ksplit; ++k) v += *reinterpret_cast<const f32x4_t*>(g.part + k * sl + q * 4);
        if (g.bias) v += *reinterpret_cast<const f32x4_t*>(g.bias + n);
        v *= g.alpha;
        if (g.res) v += *reinterpret_cast<const f32x4_t*>(g.res + m * g.ldr + n);
        float* cp = g.c + m * g.ldc + n;
        if (g.accumulate) v += *reinterpret_cast<const f32x4_t*>(cp);
        *reinterpret_cast<f32x4_t*>(cp) = v;
    }
}

// ---------------------------------------------------------------- B packing (weights, once per network)
// job j: B[n][k] = trans ? src[k * ld + n] : src[n * ld + k], n < rows, k < K ->
// planes [rows][K / 32][xh 32 | xl 32] with one scale per row, 1 / s to inv[n].
// Two launches over a (64-row block, K split, job) grid -- a 384-row operand with
// K = 12288 (the DiT patch GEMMs) would otherwise run on six workgroups: pass 1
// writes the row maxima of every K split to part[n][ks] (behind inv in the pack
// buffer), pass 2 combines them into the row scale and splits its K range
// (split 0 also writes inv).  Workgroup = 4 waves over the 32-k chunks of the
// split.  Both source layouts are read coalesced: row-major as 8 lanes x float4
// per 128-B row piece; transposed with lane = row (a 256-B row of src per load),
// the split chunk then turned into 128-B destination rows through an 8 KB LDS
// tile per wave.
constexpr int kH3rPackMax = 48;
constexpr int kH3rKSplit = 64;                 // K splits (row-max partials per row)
struct H3rPackJob { const float* src; f16* dst; float* inv; float* part; int rows, K, ld, trans, nks; };
struct H3rPackBatch { H3rPackJob j[kH3rPackMax]; };

// chunk range [c0, c1) of split ks of a job
DLCS_DEV void h3r_split_range(const H3rPackJob& jb, int ks, int& c0, int& c1) {
    const int nch = jb.K >> 5, per = (nch + jb.nks - 1) / jb.nks;
    c0 = min(nch, ks * per);
    c1 = min(nch, c0 + per);
}

__global__ void __launch_bounds__(256) h3r_rowmax_kernel(H3rPackBatch bt) {
    const H3rPackJob& jb = bt.j[blockIdx.y];
    const int n0 = blockIdx.x * 64, ks = blockIdx.z;
    if (n0 >= jb.rows || ks >= jb.nks) return;
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int c0, c1;
    h3r_split_range(jb, ks, c0, c1);
    const int rl = lane >> 3, q4 = (lane & 7) * 4;      // row-major mapping: 8 rows x 8 float4 per load
    if (jb.trans) {
        const int n = min(n0 + lane, jb.rows - 1);
        float m = 0.0f;
        for (int c = c0 + wave; c < c1; c += 4)
            for (int kk = 0; kk < 32; ++kk) m = fmaxf(m, fabsf(jb.src[(long)(c * 32 + kk) * jb.ld + n]));
        red[wave][lane] = m;
    } else {
        for (int rb = 0; rb < 8; ++rb) {
            const int n = min(n0 + rb * 8 + rl, jb.rows - 1);
            float m = 0.0f;
            for (int c = c0 + wave; c < c1; c += 4) {
                const f32x4_t v = *reinterpret_cast<const f32x4_t*>(jb.src + (long)n * jb.ld + c * 32 + q4);
                m = fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
            }
            m = lane8_max(m);
            if ((lane & 7) == 0) red[wave][rb * 8 + rl] = m;
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && n0 + (int)threadIdx.x < jb.rows) {
        const int t = threadIdx.x;
        jb.part[(long)(n0 + t) * kH3rKSplit + ks] = fmaxf(fmaxf(red[0][t], red[1][t]), fmaxf(red[2][t], red[3][t]));
    }
}

__global__ void __launch_bounds__(256) h3r_pack_kernel(H3rPackBatch bt) {
    const H3rPackJob& jb = bt.j[blockIdx.y];
    const int n0 = blockIdx.x * 64, ks = blockIdx.z;
    if (n0 >= jb.rows || ks >= jb.nks) return;
    __shared__ float scl[64];
    __shared__ __attribute__((aligned(16))) f16 tile[4][64 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int c0, c1;
    h3r_split_range(jb, ks, c0, c1);
    const int rl = lane >> 3, q4 = (lane & 7) * 4;
    if (threadIdx.x < 64) {
        const int n = min(n0 + (int)threadIdx.x, jb.rows - 1);
        float m = 0.0f;
        for (int k = 0; k < jb.nks; ++k) m = fmaxf(m, jb.part[(long)n * kH3rKSplit + k]);
        const float sc = f16x3_scale(__float_as_uint(m));
        scl[threadIdx.x] = sc;
        if (ks == 0 && n0 + (int)threadIdx.x < jb.rows) jb.inv[n0 + threadIdx.x] = 1.0f / sc;
    }
    __syncthreads();
    const long dld = (long)jb.K * 2;
    for (int c = c0 + wave; c < c1; c += 4) {
        if (jb.trans) {
            const float sc = scl[lane];
            const int n = min(n0 + lane, jb.rows - 1);
            f16* T = tile[wave];
#pragma unroll 8
            for (int kk = 0; kk < 32; ++kk) {
                const float u = jb.src[(long)(c * 32 + kk) * jb.ld + n] * sc;
                const f16 hv = (f16)u;
                T[lane * 64 + kk] = hv;
                T[lane * 64 + 32 + kk] = (f16)(u - (float)hv);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int qd = lane + 64 * i, row = qd >> 3, pc = qd & 7;
                if (n0 + row < jb.rows)
                    *reinterpret_cast<f16x8_t*>(jb.dst + (n0 + row) * dld + c * 64 + pc * 8) =
                        *reinterpret_cast<const f16x8_t*>(T + row * 64 + pc * 8);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else {
            for (int rb = 0; rb < 8; ++rb) {
                const int r = rb * 8 + rl;
                if (n0 + r >= jb.rows) continue;
                const float sc = scl[r];
                const f32x4_t v = *reinterpret_cast<const f32x4_t*>(jb.src + (long)(n0 + r) * jb.ld + c * 32 + q4);
                f16x4_t h, l;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float u = v[e] * sc;
                    const f16 hv = (f16)u;
                    h[e] = hv;
                    l[e] = (f16)(u - (float)hv);
                }
                *reinterpret_cast<f16x4_t*>(jb.dst + (n0 + r) * dld + c * 64 + q4) = h;
                *reinterpret_cast<f16x4_t*>(jb.dst + (n0 + r) * dld + c * 64 + 32 + q4) = l;
            }
        }
    }
}
