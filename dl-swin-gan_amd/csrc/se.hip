// Squeeze-excitation gate of the SE-ResNet regulariser (reference se3d.py:302-438)
// around the fused ResNet conv trunk, on the patch-blocked channels-last rows
// [B N, ld] (batch item b = rows [b N, (b + 1) N)), fp32 or -- the *_bf16 entry points of
// the four row passes -- bf16 (se_rows.h: widened on load, fp32 arithmetic, one rounding on
// store; 8 columns per 16-B access instead of 4).  The [B, C] vectors are always fp32:
//
// * dlcs_se_pool            mean[b, c] = (1 / N) sum_rows o                (GlobalAvgPool)
// * dlcs_se_gate            hidden = relu(W1 mean + b1), gate = sigmoid(W2 hidden + b2)
// * dlcs_se_scale_res_relu  out = relu(o gate[b, c] + res)
// * dlcs_se_bwd_reduce      dgate[b, c] = sum_rows g [r_next > 0] o
// * dlcs_se_gate_bwd        FC parameter gradients (+=) and dmean = (dh W1) / N
// * dlcs_se_bwd_apply       g <- g [r_next > 0] in place, dout = g gate + dmean
//
// The row passes share one geometry: a thread owns one column chunk (4 columns as
// one 16-B access when C % 4 == 0, ld % 4 == 0 and every row pointer is 16-B
// aligned, else 1 column) and walks rows strided by the number of row groups in
// its workgroup, 4 rows in flight (8 in the pool, which reads one tensor); columns
// [C, ld) are never touched.  The two reductions store one partial row per
// workgroup into the caller's workspace and a second launch sums them in a fixed
// order (no float atomics: the same input gives the same bits), because the gate
// multiplies every voxel of the block.
#include <algorithm>

#include "dlcs_common.h"
#include "se_rows.h"

namespace {

// ------------------------------------------------------------------ reductions
// part[(b G + blockIdx.x) C + c] = sum over this workgroup's rows of o (MASKED:
// of g o where r_next > 0; NaN, +-0 and negatives of r_next are dropped by a
// select, so nothing of a dropped row reaches the sum).
template <typename T, int V, bool MASKED>
__global__ void __launch_bounds__(256) se_reduce_kernel(const T* o, const T* g, const T* rn, long N, int C,
                                                        long ld, long rows_per_block, float* part) {
    __shared__ float sm[256 * V];
    const int nch = C / V;
    const int cpb = nch < 256 ? nch : 256;
    const int ngrp = 256 / cpb;
    const int ch = threadIdx.x % cpb, grp = threadIdx.x / cpb;
    const long b = blockIdx.y;
    const long r0 = b * N + (long)blockIdx.x * rows_per_block;
    const long r1 = min(b * N + N, r0 + rows_per_block);
    float* dst = part + (b * gridDim.x + blockIdx.x) * C;
    for (int cb = 0; cb < nch; cb += cpb) {
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.0f;
        if (grp < ngrp && cb + ch < nch) {
            const long col = (long)(cb + ch) * V;
            long r = r0 + grp;
            constexpr int U = MASKED ? 4 : 8;          // rows in flight: 8 x 16 B (pool), 4 x 3 x 16 B (masked)
            for (; r + (U - 1) * ngrp < r1; r += U * ngrp) {
                SeVec<V> fo[U], fg[MASKED ? U : 1], fr[MASKED ? U : 1];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const long off = (r + u * ngrp) * ld + col;
                    fo[u] = se_load<V>(o + off);
                    if constexpr (MASKED) { fg[u] = se_load<V>(g + off); fr[u] = se_load<V>(rn + off); }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        if constexpr (MASKED) acc[e] += (fr[u].v[e] > 0.0f) ? fg[u].v[e] * fo[u].v[e] : 0.0f;
                        else acc[e] += fo[u].v[e];
                    }
            }
            for (; r < r1; r += ngrp) {
                const long off = r * ld + col;
                const SeVec<V> fo = se_load<V>(o + off);
                if constexpr (MASKED) {
                    const SeVec<V> fg = se_load<V>(g + off), fr = se_load<V>(rn + off);
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[e] += (fr.v[e] > 0.0f) ? fg.v[e] * fo.v[e] : 0.0f;
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[e] += fo.v[e];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) sm[threadIdx.x * V + e] = acc[e];
        __syncthreads();
        for (int i = threadIdx.x; i < cpb * V; i += 256) {
            const int cc = i / V, e = i % V;
            if (cb + cc < nch) {
                float s = 0.0f;
                for (int q = 0; q < ngrp; ++q) s += sm[(q * cpb + cc) * V + e];
                dst[(cb + cc) * V + e] = s;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ element-wise passes
// APPLY_BWD false: out = relu(o gate + res) (a = o, bsrc = res; out may alias res).
// APPLY_BWD true : g (= gio) <- g [r_next > 0] in place, out = g gate + dmean (a = r_next).
template <typename T, int V, bool APPLY_BWD>
__global__ void __launch_bounds__(256) se_rows_kernel(const T* a, const T* bsrc, T* gio, const float* gate,
                                                      const float* dmean, T* out, long N, int C, long ld,
                                                      long rows_per_block) {
    const int nch = C / V;
    const int cpb = nch < 256 ? nch : 256;
    const int ngrp = 256 / cpb;
    const int ch = threadIdx.x % cpb, grp = threadIdx.x / cpb;
    if (grp >= ngrp) return;
    const long b = blockIdx.y;
    const long r0 = b * N + (long)blockIdx.x * rows_per_block;
    const long r1 = min(b * N + N, r0 + rows_per_block);
    for (int cb = 0; cb + ch < nch; cb += cpb) {
        const long col = (long)(cb + ch) * V;
        float s[V], d[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            s[e] = gate[b * C + col + e];
            if constexpr (APPLY_BWD) d[e] = dmean[b * C + col + e];
            else d[e] = 0.0f;
        }
        long r = r0 + grp;
        for (; r + 3 * ngrp < r1; r += 4 * ngrp) {
            SeVec<V> fa[4], fb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long off = (r + u * ngrp) * ld + col;
                fa[u] = se_load<V>(a + off);
                fb[u] = se_load<V>((APPLY_BWD ? gio : bsrc) + off);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long off = (r + u * ngrp) * ld + col;
                SeVec<V> y;
                if constexpr (APPLY_BWD) {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        if (!(fa[u].v[e] > 0.0f)) fb[u].v[e] = 0.0f;
                        y.v[e] = fb[u].v[e] * s[e] + d[e];
                    }
                    se_store<V>(gio + off, fb[u]);
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const float v = fa[u].v[e] * s[e] + fb[u].v[e];
                        y.v[e] = v > 0.0f ? v : 0.0f;
                    }
                }
                se_store<V>(out + off, y);
            }
        }
        for (; r < r1; r += ngrp) {
            const long off = r * ld + col;
            const SeVec<V> fa = se_load<V>(a + off);
            SeVec<V> fb = se_load<V>((APPLY_BWD ? gio : bsrc) + off), y;
            if constexpr (APPLY_BWD) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    if (!(fa.v[e] > 0.0f)) fb.v[e] = 0.0f;
                    y.v[e] = fb.v[e] * s[e] + d[e];
                }
                se_store<V>(gio + off, fb);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float v = fa.v[e] * s[e] + fb.v[e];
                    y.v[e] = v > 0.0f ? v : 0.0f;
                }
            }
            se_store<V>(out + off, y);
        }
    }
}

// ------------------------------------------------------------------ gate (the two FCs)
// One workgroup per batch item: mean row in LDS, one wave per hidden unit (lanes
// over C, xor-shuffle sum), then one thread per channel over the R hidden units.
__global__ void __launch_bounds__(256) se_gate_kernel(const float* mean, const float* W1, const float* b1,
                                                      const float* W2, const float* b2, int C, int R, float* hidden,
                                                      float* gate) {
    __shared__ float sm[kSeMaxC];
    __shared__ float sh[kSeMaxR];
    const long b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) sm[c] = mean[b * C + c];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave; r < R; r += 4) {
        float a = 0.0f;
        for (int c = lane; c < C; c += 64) a += W1[(long)r * C + c] * sm[c];
        a = wave_sum(a) + b1[r];
        a = a > 0.0f ? a : 0.0f;
        if (lane == 0) { sh[r] = a; hidden[b * R + r] = a; }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float z = b2[c];
        for (int r = 0; r < R; ++r) z += W2[(long)c * R + r] * sh[r];
        gate[b * C + c] = 1.0f / (1.0f + expf(-z));
    }
}

// dz2[b, c] = dgate s (1 - s);  dh[b, r] = (sum_c dz2[b, c] W2[c, r]) [hidden > 0]
__global__ void __launch_bounds__(256) se_gate_bwd_hidden_kernel(const float* dgate, const float* gate,
                                                                 const float* hidden, const float* W2, int C, int R,
                                                                 float* dz2, float* dh) {
    __shared__ float sm[kSeMaxC];
    const long b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float s = gate[b * C + c];
        const float v = dgate[b * C + c] * s * (1.0f - s);
        sm[c] = v;
        dz2[b * C + c] = v;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave; r < R; r += 4) {
        float a = 0.0f;
        for (int c = lane; c < C; c += 64) a += sm[c] * W2[(long)c * R + r];
        a = wave_sum(a);
        if (lane == 0) dh[b * R + r] = hidden[b * R + r] > 0.0f ? a : 0.0f;
    }
}

// One thread per output element, batch sums in ascending b:
//   dW1[r, c] += sum_b dh[b, r] mean[b, c]     dW2[c, r] += sum_b dz2[b, c] hidden[b, r]
//   db1[r] += sum_b dh[b, r]                   db2[c] += sum_b dz2[b, c]
//   dmean[b, c] = inv_n sum_r dh[b, r] W1[r, c]
__global__ void __launch_bounds__(256) se_gate_bwd_params_kernel(const float* dz2, const float* dh, const float* hidden,
                                                                 const float* mean, const float* W1, int B, int C,
                                                                 int R, float inv_n, float* dW1, float* db1,
                                                                 float* dW2, float* db2, float* dmean) {
    const long rc = (long)R * C;
    const long total = 2 * rc + R + C + (long)B * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        float s = 0.0f;
        if (i < rc) {
            const int r = (int)(i / C), c = (int)(i % C);
            for (int b = 0; b < B; ++b) s += dh[(long)b * R + r] * mean[(long)b * C + c];
            dW1[i] += s;
        } else if (i < 2 * rc) {
            const long j = i - rc;
            const int c = (int)(j / R), r = (int)(j % R);
            for (int b = 0; b < B; ++b) s += dz2[(long)b * C + c] * hidden[(long)b * R + r];
            dW2[j] += s;
        } else if (i < 2 * rc + R) {
            const int r = (int)(i - 2 * rc);
            for (int b = 0; b < B; ++b) s += dh[(long)b * R + r];
            db1[r] += s;
        } else if (i < 2 * rc + R + C) {
            const int c = (int)(i - 2 * rc - R);
            for (int b = 0; b < B; ++b) s += dz2[(long)b * C + c];
            db2[c] += s;
        } else {
            const long j = i - 2 * rc - R - C;
            const int b = (int)(j / C), c = (int)(j % C);
            for (int r = 0; r < R; ++r) s += dh[(long)b * R + r] * W1[(long)r * C + c];
            dmean[j] = s * inv_n;
        }
    }
}

}  // namespace

namespace {

// the row entry points on fp32 (T = float) or bf16 rows
template <typename T>
int se_pool_rows(const T* o, int64_t B, int64_t N, int64_t C, int64_t ld, float* mean, void* workspace,
                 size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(o && mean && se_rows_ok(B, N, C, ld));
    if (!se_rows_supported(B, C)) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (!ws_ok(workspace, workspace_bytes, se_partial_bytes(B, N, C))) return DLCS_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const SeGeom q = se_geom(B, N);
    float* part = (float*)workspace;
    const dim3 grid(q.G, (unsigned)B);
    if (se_vec<T>(C, ld, {o}))
        hipLaunchKernelGGL((se_reduce_kernel<T, RowVec<T>::v, false>), grid, dim3(256), 0, st, o, nullptr, nullptr,
                           (long)N, (int)C, (long)ld, q.rpb, part);
    else
        hipLaunchKernelGGL((se_reduce_kernel<T, 1, false>), grid, dim3(256), 0, st, o, nullptr, nullptr, (long)N, (int)C,
                           (long)ld, q.rpb, part);
    hipLaunchKernelGGL(se_partial_sum_kernel, dim3(cdiv(C, kSeSumCols), (unsigned)B), dim3(1024), 0, st, part, (int)q.G,
                       (int)C, (float)N, mean);
    return dlcs_launch_status();
}

template <typename T>
int se_scale_res_relu_rows(const T* o, const float* gate, const T* res, T* out, int64_t B, int64_t N,
                           int64_t C, int64_t ld, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(o && gate && res && out && out != o && se_rows_ok(B, N, C, ld));
    if (!se_rows_supported(B, C)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const SeGeom q = se_geom(B, N);
    const dim3 grid(q.G, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (se_vec<T>(C, ld, {o, res, out}))
        hipLaunchKernelGGL((se_rows_kernel<T, RowVec<T>::v, false>), grid, dim3(256), 0, st, o, res, nullptr, gate,
                           nullptr, out, (long)N, (int)C, (long)ld, q.rpb);
    else
        hipLaunchKernelGGL((se_rows_kernel<T, 1, false>), grid, dim3(256), 0, st, o, res, nullptr, gate, nullptr, out,
                           (long)N, (int)C, (long)ld, q.rpb);
    return dlcs_launch_status();
}

template <typename T>
int se_bwd_reduce_rows(const T* g, const T* r_next, const T* o, int64_t B, int64_t N, int64_t C, int64_t ld,
                       float* dgate, void* workspace, size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(g && r_next && o && dgate && se_rows_ok(B, N, C, ld));
    if (!se_rows_supported(B, C)) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (!ws_ok(workspace, workspace_bytes, se_partial_bytes(B, N, C))) return DLCS_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const SeGeom q = se_geom(B, N);
    float* part = (float*)workspace;
    const dim3 grid(q.G, (unsigned)B);
    if (se_vec<T>(C, ld, {g, r_next, o}))
        hipLaunchKernelGGL((se_reduce_kernel<T, RowVec<T>::v, true>), grid, dim3(256), 0, st, o, g, r_next, (long)N,
                           (int)C, (long)ld, q.rpb, part);
    else
        hipLaunchKernelGGL((se_reduce_kernel<T, 1, true>), grid, dim3(256), 0, st, o, g, r_next, (long)N, (int)C, (long)ld,
                           q.rpb, part);
    hipLaunchKernelGGL(se_partial_sum_kernel, dim3(cdiv(C, kSeSumCols), (unsigned)B), dim3(1024), 0, st, part, (int)q.G,
                       (int)C, 1.0f, dgate);
    return dlcs_launch_status();
}

template <typename T>
int se_bwd_apply_rows(T* g, const T* r_next, const float* gate, const float* dmean, T* dout, int64_t B,
                      int64_t N, int64_t C, int64_t ld, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(g && r_next && gate && dmean && dout && dout != g && se_rows_ok(B, N, C, ld));
    if (!se_rows_supported(B, C)) return DLCS_ERR_UNSUPPORTED_SIZE;
    const SeGeom q = se_geom(B, N);
    const dim3 grid(q.G, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (se_vec<T>(C, ld, {g, r_next, dout}))
        hipLaunchKernelGGL((se_rows_kernel<T, RowVec<T>::v, true>), grid, dim3(256), 0, st, r_next, nullptr, g, gate,
                           dmean, dout, (long)N, (int)C, (long)ld, q.rpb);
    else
        hipLaunchKernelGGL((se_rows_kernel<T, 1, true>), grid, dim3(256), 0, st, r_next, nullptr, g, gate, dmean, dout,
                           (long)N, (int)C, (long)ld, q.rpb);
    return dlcs_launch_status();
}

}  // namespace

extern "C" {

size_t dlcs_se_pool_workspace_bytes(int64_t B, int64_t N, int64_t C) {
    return (B > 0 && N > 0 && C > 0) ? se_partial_bytes(B, N, C) : 0;
}

int dlcs_se_pool(const float* o, int64_t B, int64_t N, int64_t C, int64_t ld, float* mean, void* workspace,
                 size_t workspace_bytes, dlcs_stream_t stream) {
    return se_pool_rows<float>(o, B, N, C, ld, mean, workspace, workspace_bytes, stream);
}

int dlcs_se_pool_bf16(const void* o, int64_t B, int64_t N, int64_t C, int64_t ld, float* mean, void* workspace,
                      size_t workspace_bytes, dlcs_stream_t stream) {
    return se_pool_rows<bf16>((const bf16*)o, B, N, C, ld, mean, workspace, workspace_bytes, stream);
}

int dlcs_se_gate(const float* mean, const float* W1, const float* b1, const float* W2, const float* b2, int64_t B,
                 int64_t C, int64_t R, float* hidden, float* gate, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(mean && W1 && b1 && W2 && b2 && hidden && gate && B > 0 && C > 0 && R > 0);
    if (C > kSeMaxC || R > kSeMaxR || B >= (1L << 31)) return DLCS_ERR_UNSUPPORTED_SIZE;
    hipLaunchKernelGGL(se_gate_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, mean, W1, b1, W2, b2, (int)C,
                       (int)R, hidden, gate);
    return dlcs_launch_status();
}

int dlcs_se_scale_res_relu(const float* o, const float* gate, const float* res, float* out, int64_t B, int64_t N,
                           int64_t C, int64_t ld, dlcs_stream_t stream) {
    return se_scale_res_relu_rows<float>(o, gate, res, out, B, N, C, ld, stream);
}

int dlcs_se_scale_res_relu_bf16(const void* o, const float* gate, const void* res, void* out, int64_t B, int64_t N,
                                int64_t C, int64_t ld, dlcs_stream_t stream) {
    return se_scale_res_relu_rows<bf16>((const bf16*)o, gate, (const bf16*)res, (bf16*)out, B, N, C, ld, stream);
}

size_t dlcs_se_bwd_reduce_workspace_bytes(int64_t B, int64_t N, int64_t C) {
    return (B > 0 && N > 0 && C > 0) ? se_partial_bytes(B, N, C) : 0;
}

int dlcs_se_bwd_reduce(const float* g, const float* r_next, const float* o, int64_t B, int64_t N, int64_t C, int64_t ld,
                       float* dgate, void* workspace, size_t workspace_bytes, dlcs_stream_t stream) {
    return se_bwd_reduce_rows<float>(g, r_next, o, B, N, C, ld, dgate, workspace, workspace_bytes, stream);
}

int dlcs_se_bwd_reduce_bf16(const void* g, const void* r_next, const void* o, int64_t B, int64_t N, int64_t C, int64_t ld,
                            float* dgate, void* workspace, size_t workspace_bytes, dlcs_stream_t stream) {
    return se_bwd_reduce_rows<bf16>((const bf16*)g, (const bf16*)r_next, (const bf16*)o, B, N, C, ld, dgate, workspace,
                                    workspace_bytes, stream);
}

size_t dlcs_se_gate_bwd_workspace_bytes(int64_t B, int64_t C, int64_t R) {
    return (B > 0 && C > 0 && R > 0) ? ws_align((size_t)B * C * sizeof(float)) + ws_align((size_t)B * R * sizeof(float)) : 0;
}

int dlcs_se_gate_bwd(const float* dgate, const float* gate, const float* hidden, const float* mean, const float* W1,
                     const float* W2, int64_t B, int64_t C, int64_t R, float inv_n, float* dW1, float* db1, float* dW2,
                     float* db2, float* dmean, void* workspace, size_t workspace_bytes, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(dgate && gate && hidden && mean && W1 && W2 && dW1 && db1 && dW2 && db2 && dmean && B > 0 && C > 0 &&
                   R > 0);
    if (C > kSeMaxC || R > kSeMaxR || B >= (1L << 20)) return DLCS_ERR_UNSUPPORTED_SIZE;
    if (!ws_ok(workspace, workspace_bytes, dlcs_se_gate_bwd_workspace_bytes(B, C, R))) return DLCS_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* dz2 = (float*)workspace;
    float* dh = (float*)((char*)workspace + ws_align((size_t)B * C * sizeof(float)));
    hipLaunchKernelGGL(se_gate_bwd_hidden_kernel, dim3((unsigned)B), dim3(256), 0, st, dgate, gate, hidden, W2, (int)C,
                       (int)R, dz2, dh);
    const long total = 2 * R * C + R + C + B * C;
    hipLaunchKernelGGL(se_gate_bwd_params_kernel, dim3(std::min<unsigned>(2048u, cdiv(total, 256))), dim3(256), 0, st, dz2,
                       dh, hidden, mean, W1, (int)B, (int)C, (int)R, inv_n, dW1, db1, dW2, db2, dmean);
    return dlcs_launch_status();
}

int dlcs_se_bwd_apply(float* g, const float* r_next, const float* gate, const float* dmean, float* dout, int64_t B,
                      int64_t N, int64_t C, int64_t ld, dlcs_stream_t stream) {
    return se_bwd_apply_rows<float>(g, r_next, gate, dmean, dout, B, N, C, ld, stream);
}

int dlcs_se_bwd_apply_bf16(void* g, const void* r_next, const float* gate, const float* dmean, void* dout, int64_t B,
                           int64_t N, int64_t C, int64_t ld, dlcs_stream_t stream) {
    return se_bwd_apply_rows<bf16>((bf16*)g, (const bf16*)r_next, gate, dmean, (bf16*)dout, B, N, C, ld, stream);
}

}  // extern "C"
