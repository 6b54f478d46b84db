// The fp32 GEMMs on the fp16 / fp8 matrix cores: K = 160 on two plane buffers, the NT GEMM
// with per-row scales on a packed B (h3r) and the DiT fp8 path (f8r).
#include "f16x3_common.h"

namespace {
#include "gemm_k160_f16x3.inc"
#include "gemm_h3r.inc"
#include "gemm_f8r.inc"
static long gemm_k160_tiles(long M, long N) { return (long)cdiv(M, 64) * (N / 160); }
}  // namespace

extern "C" {

size_t dlcs_gemm_k160_f16x3_workspace_bytes(int64_t M, int64_t N, int has_colsum) {
    return colsum_part_bytes(gemm_k160_tiles(M, N), has_colsum != 0);
}

int dlcs_gemm_k160_f16x3(const void* aplanes, int64_t M, const void* bplanes, int64_t N, float* C, int64_t ldc,
                         const float* bias, int act, float alpha, const float* residual, int64_t ldr, float res_scale,
                         const float* residual2, int64_t ldr2, float res2_scale, int accumulate, unsigned* out_max,
                         void* out_planes, float* colsum, const void* res_planes, const void* res2_planes,
                         void* workspace, size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(aplanes && bplanes && M > 0 && N > 0 && (act == 0 || act == 3) &&
                   (C || (out_planes && !accumulate)) && !(residual && res_planes) && !(residual2 && res2_planes));
    if (!C) ldc = N;
    if (N % 160 || ldc % 4 || !al16(aplanes) || !al16(bplanes) || !al16(C) || (bias && !al16(bias)) ||
        (residual && (ldr % 4 || !al16(residual))) || (residual2 && (ldr2 % 4 || !al16(residual2))) ||
        M * 320 >= (1L << 40))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    GemmH3Args g{};
    g.ap = (const f16*)aplanes; g.bp = (const f16*)bplanes;
    g.amax = planes_trailer(aplanes, M); g.bmax = planes_trailer(bplanes, N);
    g.c = C; g.ldc = ldc; g.bias = bias; g.act = act; g.alpha = alpha;
    g.res = residual; g.ldr = ldr; g.res_scale = res_scale;
    g.res2 = residual2; g.ldr2 = ldr2; g.res2_scale = res2_scale;
    g.accumulate = accumulate; g.M = (int)M; g.N = (int)N; g.omax = out_max;
    const long prows = M * (N / 160);                          // rows of the [M N / 160][160] view
    if (res_planes) {
        if (!al16(res_planes)) return DLCS_ERR_UNSUPPORTED_SIZE;
        g.rp = (const f16*)res_planes; g.rpmax = planes_trailer(res_planes, prows);
    }
    if (res2_planes) {
        if (!al16(res2_planes)) return DLCS_ERR_UNSUPPORTED_SIZE;
        g.rp2 = (const f16*)res2_planes; g.rp2max = planes_trailer(res2_planes, prows);
    }
    if (out_planes) {
        if (ldc != N || !al16(out_planes)) return DLCS_ERR_UNSUPPORTED_SIZE;
        g.oplanes = (f16*)out_planes; g.opmax = planes_trailer(out_planes, prows);
    }
    hipStream_t st = (hipStream_t)stream;
    const long nwg = gemm_k160_tiles(M, N);
    if (colsum) {
        if (g.row_map || nwg > (1L << 24)) return DLCS_ERR_UNSUPPORTED_SIZE;
        if (!ws_ok(workspace, workspace_bytes, colsum_part_bytes(nwg, true))) return DLCS_ERR_WORKSPACE;
        g.cpart = static_cast<float*>(workspace);
    }
    const int rc = gemm_k160_launch(g, st);
    if (rc || !colsum) return rc;
    return dlcs_internal::launch_colsum_parts(g.cpart, (int)nwg, colsum, st);
}

int dlcs_linear_k160_f16x3(const void* xplanes, int64_t M, const void* wplanes, int64_t N, float* C, int64_t ldc,
                           const float* bias, int act, const float* aux, float* aux_out, int64_t ldaux, float alpha,
                           const float* residual, int64_t ldr, const int32_t* row_map, int accumulate,
                           dlcs_stream_t stream) {
    DLCS_CHECK_ARG(xplanes && wplanes && C && M > 0 && N > 0 && act >= 0 && act <= 3 && (act != 2 || aux));
    if (N % 160 || ldc % 4 || !al16(xplanes) || !al16(wplanes) || !al16(C) || (bias && !al16(bias)) ||
        (residual && (ldr % 4 || !al16(residual))) || ((aux || aux_out) && ldaux % 4) || (aux && !al16(aux)) ||
        (aux_out && !al16(aux_out)) || M * 320 >= (1L << 40))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    GemmH3Args g{};
    g.ap = (const f16*)xplanes; g.bp = (const f16*)wplanes;
    g.amax = planes_trailer(xplanes, M); g.bmax = planes_trailer(wplanes, N);
    g.c = C; g.ldc = ldc; g.bias = bias; g.act = act; g.alpha = alpha;
    g.res = residual; g.ldr = ldr; g.res_scale = 1.0f;
    g.accumulate = accumulate; g.M = (int)M; g.N = (int)N;
    g.aux = aux; g.aux_out = aux_out; g.ldaux = ldaux; g.row_map = row_map;
    return gemm_k160_launch(g, (hipStream_t)stream);
}

size_t dlcs_h3r_pack_bytes(int64_t rows, int64_t K) {
    return (size_t)rows * K * 4 + (size_t)rows * 4 + (size_t)rows * kH3rKSplit * 4 + 256;
}

int dlcs_h3r_pack_multi(int n, const float* const* src, const int64_t* ld, const int* trans, const int64_t* rows,
                        const int64_t* K, void* const* dst, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(n >= 0 && (n == 0 || (src && ld && trans && rows && K && dst)));
    for (int i0 = 0; i0 < n; i0 += kH3rPackMax) {
        H3rPackBatch bt{};
        const int cnt = std::min(n - i0, kH3rPackMax);
        int64_t maxrows = 0;
        int maxks = 1;
        for (int j = 0; j < cnt; ++j) {
            const int i = i0 + j;
            DLCS_CHECK_ARG(src[i] && dst[i] && rows[i] > 0 && K[i] > 0 && K[i] % 32 == 0 && ld[i] > 0 &&
                           ((uintptr_t)dst[i] & 15) == 0 && (trans[i] || (ld[i] % 4 == 0 && ((uintptr_t)src[i] & 15) == 0)));
            if (rows[i] > (1 << 20) || K[i] > 16384 || rows[i] * K[i] * 4 >= (1L << 31)) return DLCS_ERR_UNSUPPORTED_SIZE;
            H3rPackJob& jb = bt.j[j];
            jb.src = src[i]; jb.dst = (f16*)dst[i]; jb.inv = (float*)((char*)dst[i] + rows[i] * K[i] * 4);
            jb.part = jb.inv + rows[i];
            jb.rows = (int)rows[i]; jb.K = (int)K[i]; jb.ld = (int)ld[i]; jb.trans = trans[i];
            // K splits: at least 4 chunks of 32 per split (one per wave), at most kH3rKSplit --
            // the packing is latency-bound (16 splits of K = 10240 ran 52 us on 96 workgroups)
            jb.nks = (int)std::max<int64_t>(1, std::min<int64_t>(kH3rKSplit, K[i] / 128));
            maxrows = std::max(maxrows, rows[i]);
            maxks = std::max(maxks, jb.nks);
        }
        const dim3 grid((unsigned)cdiv(maxrows, 64), (unsigned)cnt, (unsigned)maxks);
        hipLaunchKernelGGL(h3r_rowmax_kernel, grid, dim3(256), 0, (hipStream_t)stream, bt);
        hipLaunchKernelGGL(h3r_pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, bt);
        const int st = dlcs_launch_status();
        if (st) return st;
    }
    return 0;
}

// deep K with a plain epilogue runs split over K: at most 8 raw partial tiles [M][N]
static bool h3r_deep_k(long K, long N, int act, bool row_map, bool aux_out) {
    return N % 160 == 0 && K % 160 == 0 && K / 160 >= 16 && act == 0 && !row_map && !aux_out;
}

size_t dlcs_gemm_h3r_workspace_bytes(int64_t M, int64_t K, int64_t N, int act, int has_row_map, int has_aux_out) {
    return h3r_deep_k(K, N, act, has_row_map != 0, has_aux_out != 0) ? (size_t)8 * M * N * sizeof(float) : 0;
}

int dlcs_gemm_h3r(const float* A, int64_t M, int64_t K, int64_t lda, const void* bpacked, int64_t N, float* C,
                  int64_t ldc, const float* bias, int act, const float* aux, float* aux_out, int64_t ldaux, float alpha,
                  const float* residual, int64_t ldr, const int32_t* row_map, int accumulate, void* workspace,
                  size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(A && bpacked && C && M > 0 && N > 0 && K > 0 && act >= 0 && act <= 7 &&
                   ((act != 2 && act != 5 && act != 6) || aux) && lda >= K);
    // tile shape: N % 160 (the Swin Linears, the unembed input gradient) with K in
    // segments of 160, else N tiles of 128 or 64 with K in segments of 192, 128 or 64
    int nj = 0, nch = 0;
    if (N % 160 == 0 && K % 160 == 0) { nj = 5; nch = 5; }
    else if (N % 64 == 0 && K % 64 == 0) { nj = N % 128 == 0 ? 4 : 2; nch = K % 192 == 0 ? 6 : K % 128 == 0 ? 4 : 2; }
    if (!nj || lda % 4 || ldc % 4 || !al16(A) || !al16(bpacked) || !al16(C) || (bias && !al16(bias)) ||
        (residual && (ldr % 4 || !al16(residual))) || ((aux || aux_out) && ldaux % 4) || (aux && !al16(aux)) ||
        (aux_out && !al16(aux_out)) || M >= (1L << 31) || K > 16384 || N * K * 4 >= (1L << 31))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    if (!ws_ok(workspace, workspace_bytes,
               dlcs_gemm_h3r_workspace_bytes(M, K, N, act, row_map != nullptr, aux_out != nullptr)))
        return DLCS_ERR_WORKSPACE;
    GemmH3rArgs g{};
    g.a = A; g.lda = lda; g.M = (int)M;
    g.bp = (const f16*)bpacked; g.binv = (const float*)((const char*)bpacked + N * K * 4); g.N = (int)N;
    g.c = C; g.ldc = ldc; g.bias = bias; g.act = act; g.alpha = alpha;
    g.res = residual; g.ldr = ldr; g.row_map = row_map; g.accumulate = accumulate;
    g.aux = aux; g.aux_out = aux_out; g.ldaux = ldaux;
    g.ntn = (int)(N / (32 * nj));
    g.ntiles = (int)cdiv(M, 64) * g.ntn;
    g.nseg = (int)(K / (32 * nch));
    hipStream_t st = (hipStream_t)stream;
    // deep K with a plain epilogue (the unembed input gradient and patch-embed forward,
    // K = 10240 in 64 segments of 160 on 210 row tiles): ksplit K ranges on disjoint
    // XCD groups (8: each XCD streams its own 0.8 MB of B from its L2), raw partial
    // tiles summed in a fixed order by h3r_ksplit_reduce_kernel.  tools/embed_bench.py:
    // 272 us unsplit, 238 / 250 / 235 us at 2 / 4 / 8 ranges (x6 NT GEMM: 290 us)
    g.ksplit = 1;
    if (h3r_deep_k(K, N, act, row_map != nullptr, aux_out != nullptr)) {
        static const int ks_env = [] { const char* e = dlcs_knob("DLCS_H3R_KSPLIT"); return e ? atoi(e) : 0; }();
        const int ks = ks_env == 1 || ks_env == 2 || ks_env == 4 || ks_env == 8 ? ks_env : 8;
        if (ks > 1) {
            g.part = static_cast<float*>(workspace);    // ks <= 8 partial tiles
            g.ksplit = ks;
        }
    }
    g.per_xcd = (int)cdiv(g.ntiles, 8 / g.ksplit);
    const dim3 grid((unsigned)(8 * g.per_xcd)), block(512);
    if (nj == 5) {
        // K = 480 / 640 in 160-wide segments: the per-segment fold (fp32 VALU add of the
        // segment's tile) keeps the matrix core's accumulate chain at 15 MFMAs
        g.nseg = (int)(K / 160);
        if (g.nseg == 1) hipLaunchKernelGGL((gemm_h3r_kernel<5, 5, false>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((gemm_h3r_kernel<5, 5, true>), grid, block, 0, st, g);
        if (g.ksplit > 1)
            hipLaunchKernelGGL(h3r_ksplit_reduce_kernel, dim3((unsigned)std::min<long>(2048, cdiv(M * N / 4, 256))),
                               dim3(256), 0, st, g);
    } else if (nj == 4) {
        if (nch == 6) hipLaunchKernelGGL((gemm_h3r_kernel<6, 4, true>), grid, block, 0, st, g);
        else if (nch == 4) hipLaunchKernelGGL((gemm_h3r_kernel<4, 4, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((gemm_h3r_kernel<2, 4, true>), grid, block, 0, st, g);
    } else {
        if (nch == 6) hipLaunchKernelGGL((gemm_h3r_kernel<6, 2, true>), grid, block, 0, st, g);
        else if (nch == 4) hipLaunchKernelGGL((gemm_h3r_kernel<4, 2, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((gemm_h3r_kernel<2, 2, true>), grid, block, 0, st, g);
    }
    return dlcs_launch_status();
}

int dlcs_f8r_quant(const float* x, int64_t rows, int64_t K, int64_t ld, void* q, float* inv, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(x && q && inv && rows > 0 && K > 0 && ld >= K);
    if (K % 4 || ld % 4 || ((uintptr_t)x & 15) || ((uintptr_t)q & 3) || K > (1 << 20))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    hipLaunchKernelGGL(quant_f8r_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, (long)rows, (int)K,
                       (long)ld, (unsigned*)q, inv);
    return dlcs_launch_status();
}

int dlcs_gemm_f8r(const void* aq, const float* ainv, int64_t M, int64_t K, const void* bq, const float* binv,
                  int64_t N, float* C, int64_t ldc, const float* bias, int act, float* aux_out, int64_t ldaux,
                  float alpha, const float* residual, int64_t ldr, const int32_t* row_map, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(aq && ainv && bq && binv && C && M > 0 && N > 0 && K > 0 && (act == 0 || act == 1 || act == 4));
    if (K % 64 || N % 64 || ((uintptr_t)aq & 15) || ((uintptr_t)bq & 15) || M * K >= (1L << 40))
        return DLCS_ERR_UNSUPPORTED_SIZE;
    GemmF8rArgs g{};
    g.a = (const unsigned char*)aq; g.ainv = ainv; g.M = (int)M;
    g.b = (const unsigned char*)bq; g.binv = binv; g.N = (int)N; g.K = (int)K;
    g.c = C; g.ldc = ldc; g.bias = bias; g.act = act; g.alpha = alpha;
    g.res = residual; g.ldr = ldr; g.row_map = row_map; g.aux_out = aux_out; g.ldaux = ldaux;
    hipLaunchKernelGGL(gemm_f8r_kernel, dim3(cdiv(M, 64), (unsigned)(N / 64)), dim3(256), 0, (hipStream_t)stream, g);
    return dlcs_launch_status();
}

}  // extern "C"
