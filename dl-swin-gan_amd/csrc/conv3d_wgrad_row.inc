// ---------------------------------------------------------------- wgrad, any channel pair (bf16)
// The weight gradient of the conv trunks (ResNet / SE / CBAM, 64 features) in bf16:
//   dW[tap][co][ci] += sum_v g[v][co] x[v + off(tap)][ci]
// for cout_pad = 32 MT (MT 1..5) and cin_pad = 32 NT (NT 1, 2, 4, 5), after the model of the
// 160 x 160 kernel above.
//
// Tiling.  One workgroup = tap row (kd, kh) x voxel range.  Its 3 MT waves = 3 kw taps x MT
// 32-row co tiles; a wave owns dW[tap][32 co][all cin_pad ci] as NT 32x32 accumulators
// (v_mfma_f32_32x32x16_bf16, 16 NT fp32 registers per lane: 32 at 64 x 64, 80 at most), so
// at 64 x 64 a workgroup of 6 waves owns the whole tap row (3 x 4096 accumulators).  K =
// voxels, one 64-voxel patch at a time: the g rows [64][cout_pad] and the tap row's x halo
// [4 t][4 y][6 x][cin_pad] -- shared by the 3 kw taps, 96 rows instead of 3 x 64 -- are
// staged in LDS in their channel-contiguous layout from register-prefetched 16-B loads (the
// next patch's loads are in flight while this one is multiplied) and read back
// voxel-contiguous with ds_read_b64_tr_b16.  That read is served in two groups of 32 lanes
// over 64 banks; a group is 4 consecutive rows x 32 channels (16 dwords), so a row stride of
// 16 or 48 dwords mod 64 puts the four rows on disjoint banks: rows of an even number of
// 32-channel tiles are padded by 32 bf16, odd ones (32, 96, 160 channels) are already there.
// A wave reads 1 A and NT B fragments per NT MFMAs and k-step.
//
// Budget at 64 x 64 (MT = NT = 2): 384 threads, LDS (64 + 96) x 96 x 2 B = 30,720 B, 32
// accumulators + 4 x 4 staging registers per lane: several workgroups per CU.  The largest
// instance (MT 5, NT 4) has 960 threads (15 waves, so <= 128 VGPRs) and 64 accumulators.
//
// Flush: fp32 atomics per (range, tap row) workgroup, as conv3d_wgrad_tr_kernel -- not
// run-to-run deterministic in the last bits.  The 9 tap rows of a range sit on one XCD
// (blockIdx % 8) so the re-reads of g and x by the other 8 hit that XCD's L2.

DLCS_DEV Frag8<bf16> tr_rows(const bf16* a0, const bf16* a1) {
    typedef __attribute__((address_space(3))) v4s lds_v4s;
    typedef short v8s __attribute__((ext_vector_type(8)));
    const v4s r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(const_cast<bf16*>(a0)));
    const v4s r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(const_cast<bf16*>(a1)));
    const v8s both = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3]};
    Frag8<bf16> f;
    f.v = __builtin_bit_cast(bf16x8, both);
    return f;
}

template <int MT, int NT>
__global__ void __launch_bounds__(MT * 192) conv3d_wgrad_row_kernel(WgradArgs a, int nrange, long ppr) {
    constexpr int NTHR = MT * 192;
    constexpr int COP = MT * 32, CIP = NT * 32;
    constexpr int GLD = COP + (MT % 2 ? 0 : 32), XLD = CIP + (NT % 2 ? 0 : 32);   // 16 or 48 dwords mod 64
    constexpr int GCH = 64 * (COP / 8), XCH = 96 * (CIP / 8);      // 16-B pieces of a patch
    constexpr int PER = (GCH + XCH + NTHR - 1) / NTHR;
    __shared__ __attribute__((aligned(16))) bf16 Gs[64 * GLD];     // g rows of the patch
    __shared__ __attribute__((aligned(16))) bf16 Xs[96 * XLD];     // x halo rows (4 t, 4 y) x 6 x

    const int b = blockIdx.x, xg = b & 7, slot = b >> 3;
    const int range = xg + 8 * (slot / 9), grp = slot % 9;
    if (range >= nrange) return;
    const int kd = grp / 3 - 1, kh = grp % 3 - 1;
    const int nT = a.D >> 2, nY = a.H >> 2, nX = a.W >> 2;
    const long npatch = (long)a.B * nT * nY * nX;
    const long p0 = (long)range * ppr;
    const long p1 = min(npatch, p0 + ppr);
    const bf16* in = reinterpret_cast<const bf16*>(a.in);
    const bf16* g = reinterpret_cast<const bf16*>(a.g);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kwi = wave / MT, mt = wave % MT;

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = (f32x16)0.0f;

    // (b, t, y, x) of the next patch to load: decoded once (64-bit divisions), then advanced with
    // carries -- the loads of a patch are issued in patch order
    int px = (int)(p0 % nX), py = (int)((p0 / nX) % nY), pt = (int)((p0 / ((long)nX * nY)) % nT);
    int bb = (int)(p0 / ((long)nX * nY * nT));
    Frag8<bf16> rr[PER];
    auto load_chunk = [&](long patch) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = threadIdx.x + k * NTHR;
            rr[k] = zero8<bf16>();
            if (c < GCH) {
                const int vl = c / (COP / 8), c8 = (c % (COP / 8)) * 8;
                if (c8 < a.Cout) rr[k] = load8<bf16>(g + (patch * 64 + vl) * a.g_ld + c8);
            } else if (c < GCH + XCH) {
                const int cx = c - GCH;
                const int hr = cx / (CIP / 8), c8 = (cx % (CIP / 8)) * 8;
                const int ty = hr / 6, xh = hr - ty * 6;
                const int t = pt * 4 + (ty >> 2) + kd, y = py * 4 + (ty & 3) + kh, x = px * 4 + xh - 1;
                if (c8 < a.Cin && t >= 0 && t < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W)
                    rr[k] = load8<bf16>(in + brow(bb, t, y, x, nT, nY, nX) * a.cin_ld + c8);
            }
        }
        if (++px == nX) {
            px = 0;
            if (++py == nY) {
                py = 0;
                if (++pt == nT) { pt = 0; ++bb; }
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = threadIdx.x + k * NTHR;
            if (c < GCH) {
                const int vl = c / (COP / 8), c8 = (c % (COP / 8)) * 8;
                Frag8<bf16> f = rr[k];
#pragma unroll
                for (int e = 0; e < 8; ++e) if (c8 + e >= a.Cout) f.v[e] = (bf16)0.0f;
                *reinterpret_cast<bf16x8*>(Gs + vl * GLD + c8) = f.v;
            } else if (c < GCH + XCH) {
                const int cx = c - GCH;
                const int hr = cx / (CIP / 8), c8 = (cx % (CIP / 8)) * 8;
                Frag8<bf16> f = rr[k];
#pragma unroll
                for (int e = 0; e < 8; ++e) if (c8 + e >= a.Cin) f.v[e] = (bf16)0.0f;
                *reinterpret_cast<bf16x8*>(Xs + hr * XLD + c8) = f.v;
            }
        }
    };

    // lane -> rows of a transposed read: 16-lane group (hh, c16) covers voxels 8 hh .. 8 hh + 7 of
    // a 16-voxel k-step and channels 16 c16 .. + 15; q = row of a 4-row read, p4 = channel quad.
    // Voxel v = 16 kk + 8 hh + 4 h + q is g row v and halo row (4 kk + 2 hh + h) * 6 + q + kwi.
    const int hh = lane >> 5, c16 = (lane >> 4) & 1, q = (lane >> 2) & 3, p4 = (lane & 3) * 4;
    const bf16* Ga = Gs + (8 * hh + q) * GLD + mt * 32 + 16 * c16 + p4;
    const bf16* Xa = Xs + (12 * hh + q + kwi) * XLD + 16 * c16 + p4;

    if (p0 < p1) load_chunk(p0);
    for (long patch = p0; patch < p1; ++patch) {
        __syncthreads();
        store_chunk();
        __syncthreads();
        if (patch + 1 < p1) load_chunk(patch + 1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {                // 4 x 16 voxels
            const Frag8<bf16> af = tr_rows(Ga + kk * 16 * GLD, Ga + (kk * 16 + 4) * GLD);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const Frag8<bf16> bfr = tr_rows(Xa + kk * 24 * XLD + j * 32, Xa + (kk * 24 + 6) * XLD + j * 32);
                mfma32(acc[j], af, bfr);
            }
        }
    }
    // flush: dw packed [27][co_pad][ci_pad]; C/D row -> co, col -> ci
    const int tap = grp * 3 + kwi;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int ci = j * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = mt * 32 + acc_row(r, lane);
            if (co < a.Cout && ci < a.Cin) atomicAdd(a.dw + ((long)tap * COP + co) * CIP + ci, acc[j][r]);
        }
    }
}

// (5, 5), (5, 1) and (1, 5) stay with conv3d_wgrad_tr_kernel, which had them before
inline int wgrad_row_launch(const WgradArgs& a, int nrange, long ppr, hipStream_t st) {
    const int mt = a.cout_pad / 32, nt = a.cin_pad / 32;
    const dim3 grid((unsigned)((nrange + 7) / 8 * 8 * 9)), block((unsigned)(mt * 192));
#define DLCS_WG_ROW(M, N) \
    case M * 8 + N: hipLaunchKernelGGL((conv3d_wgrad_row_kernel<M, N>), grid, block, 0, st, a, nrange, ppr); break
    switch (mt * 8 + nt) {
        DLCS_WG_ROW(1, 1); DLCS_WG_ROW(1, 2); DLCS_WG_ROW(1, 4);
        DLCS_WG_ROW(2, 1); DLCS_WG_ROW(2, 2); DLCS_WG_ROW(2, 4); DLCS_WG_ROW(2, 5);
        DLCS_WG_ROW(3, 1); DLCS_WG_ROW(3, 2); DLCS_WG_ROW(3, 4); DLCS_WG_ROW(3, 5);
        DLCS_WG_ROW(4, 1); DLCS_WG_ROW(4, 2); DLCS_WG_ROW(4, 4); DLCS_WG_ROW(4, 5);
        DLCS_WG_ROW(5, 2); DLCS_WG_ROW(5, 4);
        default: return DLCS_ERR_UNSUPPORTED_SIZE;
    }
#undef DLCS_WG_ROW
    return dlcs_launch_status();
}
