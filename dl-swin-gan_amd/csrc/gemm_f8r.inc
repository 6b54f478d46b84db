// ---------------------------------------------------------------- fp8 (OCP e4m3) token GEMM, row-scaled (f8r)
// Included by gemm_f16x3.hip.  The fp8 MFMA path of the diffusion
// denoisers (BASELINE config 5, DiT / Latte token Linears, inference):
//   C[row(m), n] = alpha act(sum_k A[m, k] B[n, k] / (s_a[m] s_b[n]) + bias[n]) + res[row(m), n]
// with A and B quantised to e4m3 by dlcs_f8r_quant: one power-of-two scale per
// row (max |s x| in (128, 256], under e4m3's 448), 1 / s per row kept in fp32,
// so only the 3-bit mantissa rounding remains (per-element relative error
// <= 2^-4; NRMSE of a K-term product ~3-5e-2 -- the budget is stated in the tests).
// v_mfma_f32_16x16x32_fp8_fp8 (lane l: A[row l & 15][k = 8 (l >> 4) + j], 8 bytes),
// one product per k-step instead of the three of the f16x3 fp32 split.
// Tile 64 x 64, 4 waves of 16 rows x 4 column tiles, K chunks of 64 bytes per
// row double-buffered through LDS (global -> registers -> LDS); 16 KB of LDS.
DLCS_DEV float f8r_scale(float m) {
    if (!(m > 0.0f) || !(m < 3.0e38f)) return 1.0f;
    int e;
    const float f = frexpf(m, &e);                  // m = f 2^e, f in [0.5, 1)
    int k = 8 - (f == 0.5f ? e - 1 : e);            // 8 - ceil(log2 m): max |s x| <= 256
    k = k < -100 ? -100 : (k > 100 ? 100 : k);
    return ldexpf(1.0f, k);
}

// rows x K fp32 (row stride ld, K % 4 == 0) -> q [rows][K] e4m3, inv [rows] = 1 / s
__global__ void __launch_bounds__(256) quant_f8r_kernel(const float* x, long rows, int K, long ld, unsigned* q,
                                                        float* inv) {
    const int lane = threadIdx.x & 63;
    const long r = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + r * ld;
    float m = 0.0f;
    for (int k = 4 * lane; k < K; k += 256) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(xr + k);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
    m = wave_max(m);
    const float s = f8r_scale(m);
    if (lane == 0) inv[r] = 1.0f / s;
    unsigned* qr = q + r * (K / 4);
    for (int k = 4 * lane; k < K; k += 256) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(xr + k);
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * s, v[1] * s, 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * s, v[3] * s, w, true);
        qr[k / 4] = (unsigned)w;
    }
}

struct GemmF8rArgs {
    const unsigned char* a; const float* ainv; int M;
    const unsigned char* b; const float* binv; int N; int K;
    float* c; long ldc;
    const float* bias; int act; float alpha;
    const float* res; long ldr;
    const int* row_map;
    float* aux_out; long ldaux;
};

__global__ void __launch_bounds__(256) gemm_f8r_kernel(GemmF8rArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned char smem_f8[2][2][64 * 64];   // [slot][A | B][row][64 B]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const int lr = threadIdx.x >> 2, lp = threadIdx.x & 3;        // loader: row, 16-B piece
    const unsigned char* arow = g.a + (long)min(m0 + lr, g.M - 1) * g.K + lp * 16;
    const unsigned char* brow = g.b + (long)(n0 + lr) * g.K + lp * 16;
    const int nch = g.K / 64;
    // 16-B pieces XOR-swizzled by (row >> 2) & 3 so the 16 rows of an operand read spread over the banks
    const int lsw = lr * 64 + ((lp ^ ((lr >> 2) & 3)) << 4);
    uint4 ra = *reinterpret_cast<const uint4*>(arow);
    uint4 rb = *reinterpret_cast<const uint4*>(brow);
    *reinterpret_cast<uint4*>(&smem_f8[0][0][lsw]) = ra;
    *reinterpret_cast<uint4*>(&smem_f8[0][1][lsw]) = rb;
    __syncthreads();
    f32x4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4_t)0.0f;
    const int vq = lane & 15, cq = lane >> 4;
    for (int c = 0; c < nch; ++c) {
        const int cur = c & 1;
        if (c + 1 < nch) {
            ra = *reinterpret_cast<const uint4*>(arow + (c + 1) * 64);
            rb = *reinterpret_cast<const uint4*>(brow + (c + 1) * 64);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // byte 32 s + 8 cq of the row = piece 2 s + (cq >> 1), offset 8 (cq & 1)
            const int pa = 2 * s + (cq >> 1);
            const int ar = wave * 16 + vq;
            const long av = *reinterpret_cast<const long*>(&smem_f8[cur][0][ar * 64 + ((pa ^ ((ar >> 2) & 3)) << 4) +
                                                                         8 * (cq & 1)]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int br = 16 * j + vq;
                const long bv = *reinterpret_cast<const long*>(&smem_f8[cur][1][br * 64 + ((pa ^ ((br >> 2) & 3)) << 4) +
                                                                             8 * (cq & 1)]);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(av, bv, acc[j], 0, 0, 0);
            }
        }
        if (c + 1 < nch) {
            *reinterpret_cast<uint4*>(&smem_f8[cur ^ 1][0][lsw]) = ra;
            *reinterpret_cast<uint4*>(&smem_f8[cur ^ 1][1][lsw]) = rb;
        }
        __syncthreads();
    }
    float ib[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ib[j] = g.binv[n0 + 16 * j + vq];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long m = m0 + wave * 16 + 4 * cq + r;
        if (m >= g.M) continue;
        long orow = m;
        if (g.row_map) {
            orow = g.row_map[m];
            if (orow < 0) continue;
        }
        const float ia = g.ainv[m];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long n = n0 + 16 * j + vq;
            float v = acc[j][r] * (ia * ib[j]);
            if (g.bias) v += g.bias[n];
            if (g.act == 4) {
                if (g.aux_out) g.aux_out[m * g.ldaux + n] = v;
                v = gelu_tanh(v);
            } else if (g.act == 1) {
                if (g.aux_out) g.aux_out[m * g.ldaux + n] = v;
                v = gelu_erf(v);
            }
            v *= g.alpha;
            if (g.res) v += g.res[orow * g.ldr + n];
            g.c[orow * g.ldc + n] = v;
        }
    }
}
