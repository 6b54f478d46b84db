// Fused shifted-window multi-head self-attention (gfx950): vst:139-170
// (WindowAttention3D.forward) after the qkv projection and before proj:
//
//   S = (scale q) k^T + B[rpi(i, j)] + mask(i, j);  P = softmax_j(S);  O = P v
//
// per (window, head); the relative-position index rpi and the -100 shift mask
// (vst:342-355) are recomputed from token coordinates / region labels, never
// materialised; P never leaves the chip (the reference keeps [nW,8,448,448]).
//
// Forward: one workgroup per (window, head, query group); each wave owns a
// 32-query block and computes S^T = K Q^T with v_mfma 32x32 (keys on the
// accumulator rows, queries on lanes, so the softmax row statistics are
// in-lane), two passes (max/sum, then P V) with P fed to the P V MFMA straight
// from the accumulator registers (A operand of Z = X^T V).  Writes O and the
// row log-sum-exp.
//
// Backward: one workgroup per (window, head, key group); each wave owns a
// 32-key block, sweeps the query blocks (staged once per workgroup) and keeps
// dK, dV in registers; dQ is reduced across waves in LDS and across key groups
// with fp32 atomics; dS is scattered into an LDS copy of the head's bias-table
// column (the relative_position_bias_table gradient), flushed with atomics.
#include "dlcs_common.h"

#include <algorithm>
#include <cstdlib>

namespace {

template <typename T> struct AttnCfg;
template <> struct AttnCfg<bf16> { static constexpr int KLD = 40, BWD_WAVES = 7; };
template <> struct AttnCfg<float> { static constexpr int KLD = 36, BWD_WAVES = 5; };

struct AttnArgs {
    const void* qkv;      // [rows, 3C] T, rows = nwin * N (window order)
    const void* o;        // [rows, C]  T  (bwd)
    const void* dout;     // [rows, C]  T  (bwd)
    void* out;            // [rows, C]  T  (fwd)
    float* lse;           // [nwin, heads, N]
    const float* table;   // [nrel, heads]
    float* dqkv;          // [rows, 3C] fp32 (bwd; dQ part accumulated atomically -> zero it first)
    float* dtable;        // [nrel, heads] fp32 (bwd, accumulated)
    const int32_t* labels;// [rows] region labels (shifted blocks) or null
    const float* mask;    // explicit additive mask [mask_nw, N, N] (vst:157-160 API form) or null
    int mask_nw;
    int nwin, N, heads, hd, nrel;
    int wd0, wh0, ww0;    // constructed window (relative-position numbering)
    float scale;
    int nloop;            // h3 kernels: token blocks the main loops visit (diagnostic cut, default all)
    int exp;              // DIAG build: timing experiments (DLCS_ATTN_EXP bits; results invalid), else 0
};


// Staging loads with a bounds predicate read through a pointer selected between
// the element and a zero block, so the load itself is unconditional: a load
// under `if (ok)` compiles to a branch with its own vmcnt(0) wait, which
// serialised the staging of a workgroup on global-memory latency.
__device__ __attribute__((aligned(16))) unsigned g_attn_zero[4] = {0u, 0u, 0u, 0u};
DLCS_DEV uint2 ldz8(const void* p, bool ok) {
    return *reinterpret_cast<const uint2*>(ok ? p : static_cast<const void*>(g_attn_zero));
}
DLCS_DEV float ldzf(const float* p, bool ok) {
    return *(ok ? p : reinterpret_cast<const float*>(g_attn_zero));
}
DLCS_DEV int ldzi(const int32_t* p, bool ok) {
    return *(ok ? p : reinterpret_cast<const int32_t*>(g_attn_zero));
}

// B operand (col = token on the lane, k = d = 16 st + 8 hh + j) from a global [rows][ld] matrix
DLCS_DEV void head_frags(Frag8<bf16> (&f)[2], const bf16* src, long ld, long row, int col0, bool valid, int hd, int hh,
                         float sc) {
    uint2 raw[2][2];
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int d0 = 16 * st + 8 * hh + 4 * g;       // hd % 4 == 0: a 4-run is all in or all out
            raw[st][g] = ldz8(src + row * ld + col0 + d0, valid && d0 < hd);
        }
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const bf16* b = reinterpret_cast<const bf16*>(&raw[st][g]);
#pragma unroll
            for (int e = 0; e < 4; ++e) f[st].v[4 * g + e] = (bf16)((float)b[e] * sc);
        }
}

// rel_index(q, k) = term(q) - term(k) + c0 with term(t) = (d * (2wh0-1) + h) * (2ww0-1) + w
// of token t's (d, h, w) in the constructed window: packed per token together
// with its region label (< 32) so the score loop needs no integer division.
DLCS_DEV int rel_term(int t, const AttnArgs& a) {
    const int hw = a.wh0 * a.ww0;
    const int d = t / hw, h = (t / a.ww0) % a.wh0, w = t % a.ww0;
    return (d * (2 * a.wh0 - 1) + h) * (2 * a.ww0 - 1) + w;
}
DLCS_DEV int rel_c0(const AttnArgs& a) {
    return ((a.wd0 - 1) * (2 * a.wh0 - 1) + (a.wh0 - 1)) * (2 * a.ww0 - 1) + (a.ww0 - 1);
}

// 4 consecutive elements (8 B bf16 / 16 B fp32) as floats; p must be aligned
DLCS_DEV void load4f(const bf16* p, float (&v)[4]) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    const bf16* b = reinterpret_cast<const bf16*>(&u);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = to_f(b[i]);
}
DLCS_DEV void load4f(const float* p, float (&v)[4]) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
}

// 8 elements of a fragment gathered as two runs of 4 consecutive values:
// elements 0-3 from p0[0..3], 4-7 from p1[0..3]
template <typename T>
DLCS_DEV Frag8<T> load4x2(const T* p0, const T* p1) {
    Frag8<T> f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { f.v[i] = p0[i]; f.v[4 + i] = p1[i]; }
    return f;
}

// bias-table column of head h -> LDS (and a zeroed gradient copy): 8 loads in
// flight per thread instead of one load -> store round trip per element
DLCS_DEV void stage_bias(float* bias_s, float* gbias_s, const float* table, int nrel, int heads, int h) {
    for (int base = 0; base < nrel; base += 8 * (int)blockDim.x) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + threadIdx.x + k * blockDim.x;
            v[k] = ldzf(table + (long)i * heads + h, i < nrel);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + threadIdx.x + k * blockDim.x;
            if (i < nrel) {
                bias_s[i] = v[k];
                if (gbias_s) gbias_s[i] = 0.0f;
            }
        }
    }
}

// additive mask of (q, key): MM 1 = shifted-window region labels (-100 when
// they differ), 2 = explicit [mask_nw, N, N] mask (callers pass in-range q, key)
template <int MM>
DLCS_DEV float mask_term(const AttnArgs& a, int w, int q, int key, int info_q, int info_k) {
    if (MM == 1) return ((info_q ^ info_k) & 31) ? -100.0f : 0.0f;
    if (MM == 2) return a.mask[((long)(w % a.mask_nw) * a.N + q) * a.N + key];
    return 0.0f;
}

constexpr int FWD_WAVES = 4;
constexpr int kBins = 128;        // local table-gradient bins per wave half (bwd)

template <typename T>
__global__ void __launch_bounds__(FWD_WAVES * 64) attn_fwd_kernel(AttnArgs a) {
    constexpr int KLD = AttnCfg<T>::KLD;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int N = a.N, hd = a.hd, C = a.heads * a.hd;
    const int Np = (N + 31) & ~31;
    const int VLD = Np + 8;
    T* Ks = reinterpret_cast<T*>(smem_raw);                      // [Np][KLD]
    T* Vt = Ks + Np * KLD;                                        // [hd + 1][VLD]
    float* bias_s = reinterpret_cast<float*>(Vt + (hd + 1) * VLD); // [nrel]
    int* lab_s = reinterpret_cast<int*>(bias_s + a.nrel);        // [Np]

    const int w = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const T* qkv = reinterpret_cast<const T*>(a.qkv);
    const long row0 = (long)w * N;
    // ---- stage K (row-major, zero pad), V^T, bias column, per-key (rel term, label)
    // hd % 4 == 0 (checked by the host): 4-element vector loads of K and V rows
    const int hq = hd / 4;
    for (int i = threadIdx.x; i < Np * (KLD / 4); i += blockDim.x) {
        const int key = i / (KLD / 4), c = i % (KLD / 4);
        float kv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, vv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (key < N && c < hq) {
            load4f(qkv + (row0 + key) * 3 * C + C + h * hd + 4 * c, kv);
            load4f(qkv + (row0 + key) * 3 * C + 2 * C + h * hd + 4 * c, vv);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) Ks[key * KLD + 4 * c + e] = from_f<T>(kv[e]);
        if (c < hq) {
#pragma unroll
            for (int e = 0; e < 4; ++e) Vt[(4 * c + e) * VLD + key] = from_f<T>(vv[e]);
        }
    }
    for (int i = threadIdx.x; i < VLD; i += blockDim.x) Vt[hd * VLD + i] = from_f<T>(0.0f);
    for (int i = threadIdx.x; i < hd * (VLD - Np); i += blockDim.x)
        Vt[(i / (VLD - Np)) * VLD + Np + i % (VLD - Np)] = from_f<T>(0.0f);
    stage_bias(bias_s, nullptr, a.table, a.nrel, a.heads, h);
    for (int i = threadIdx.x; i < Np; i += blockDim.x)
        lab_s[i] = i < N ? (rel_term(i, a) << 5) | (a.labels ? a.labels[row0 + i] : 0) : 0;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qb = blockIdx.y * FWD_WAVES + wave;
    const int nqb = Np / 32;
    if (qb >= nqb) return;
    const int hh = lane >> 5;
    const int q = qb * 32 + (lane & 31);
    const bool qvalid = q < N;
    // Q fragments (B operand of S^T = K Q^T), scaled (vst:149)
    Frag8<T> qf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = kk * 16 + 8 * hh + j;
            float v = 0.0f;
            if (qvalid && d < hd) v = to_f(qkv[(row0 + q) * 3 * C + h * hd + d]) * a.scale;
            qf[kk].v[j] = from_f<T>(v);
        }
    }
    const int qlab = lab_s[q < Np ? q : 0] & 31;
    const int fq = (qvalid ? rel_term(q, a) : 0) + rel_c0(a);
    const int nkb = Np / 32;

    auto score_tile = [&](int kb, f32x16& s) {
        s = (f32x16)0.0f;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const Frag8<T> kf = load8<T>(Ks + (kb * 32 + (lane & 31)) * KLD + kk * 16 + 8 * hh);
            mfma32(s, kf, qf[kk]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kb * 32 + acc_row(r, lane);
            if (key < N && qvalid) {
                const int info = lab_s[key];
                float v = s[r] + bias_s[fq - (info >> 5)];
                if (a.labels && (info & 31) != qlab) v += -100.0f;
                if (a.mask) v += a.mask[((long)(w % a.mask_nw) * N + q) * N + key];
                s[r] = v;
            } else {
                s[r] = -INFINITY;
            }
        }
    };

    // pass 1: row max / sum (per lane = per query, over this lane-half's keys)
    float m = -INFINITY, l = 0.0f;
    for (int kb = 0; kb < nkb; ++kb) {
        f32x16 s;
        score_tile(kb, s);
        float tm = m;
#pragma unroll
        for (int r = 0; r < 16; ++r) tm = fmaxf(tm, s[r]);
        float acc = 0.0f;
        if (tm != -INFINITY) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc += __expf(s[r] - tm);
            l = l * __expf(m - tm) + acc;   // m = -inf -> exp(-inf) = 0
            m = tm;
        }
    }
    {   // combine the two lane halves (same query, disjoint keys)
        const float mo = xor32_peer(m), lo = xor32_peer(l);
        const float mn = fmaxf(m, mo);
        if (mn == -INFINITY) { m = 0.0f; l = 1.0f; }
        else { l = l * __expf(m - mn) + lo * __expf(mo - mn); m = mn; }
    }
    const float inv_l = 1.0f / l;

    // pass 2: O = P V with P straight from the accumulator (Z = X^T V)
    f32x16 z = (f32x16)0.0f;
    for (int kb = 0; kb < nkb; ++kb) {
        f32x16 s;
        score_tile(kb, s);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            Frag8<T> pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf.v[j] = from_f<T>(__expf(s[8 * st + j] - m) * inv_l);
            const int d = min(lane & 31, hd);
            const T* vrow = Vt + d * VLD + kb * 32 + 16 * st + 4 * hh;
            const Frag8<T> vf = load4x2<T>(vrow, vrow + 8);
            mfma32(z, pf, vf);
        }
    }
    // write O (rows q in registers, cols d on lanes) and the log-sum-exp
    T* out = reinterpret_cast<T*>(a.out);
    const int d = lane & 31;
    if (d < hd) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = qb * 32 + acc_row(r, lane);
            if (qq < N) out[(row0 + qq) * C + h * hd + d] = from_f<T>(z[r]);
        }
    }
    if (hh == 0 && qvalid) a.lse[((long)w * a.heads + h) * N + q] = m + __logf(l);
}

// ---------------------------------------------------------------- forward, single pass (bf16)
// One workgroup per (window, head, half of the query blocks); each wave owns
// 32-query blocks.  S^T = K Q^T (keys on accumulator rows, queries on lanes)
// and O^T = V^T P^T with P^T taken straight from the S^T accumulator as the B
// operand (its key order matched by the V^T fragment gather), so the softmax
// statistics AND the output accumulator of a query live in one lane: online
// softmax with a lane-wise rescale, one pass over the keys, exp once per score.
template <int MM>
__global__ void __launch_bounds__(1024) attn_fwd_v2_kernel(AttnArgs a) {
    constexpr int KLD = 40;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int N = a.N, hd = a.hd, C = a.heads * a.hd;
    const int Np = (N + 31) & ~31;
    const int VLD = Np + 8;
    bf16* Ks = reinterpret_cast<bf16*>(smem_raw);                        // [Np][KLD]
    bf16* Vt = Ks + Np * KLD;                                             // [hd + 1][VLD]
    float* bias_s = reinterpret_cast<float*>(Vt + (hd + 1) * VLD);        // [nrel]
    int* lab_s = reinterpret_cast<int*>(bias_s + a.nrel);                // [Np] (rel term << 5 | label)

    const int w = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const bf16* qkv = reinterpret_cast<const bf16*>(a.qkv);
    const long row0 = (long)w * N;
    const int hq = hd / 4;
    // K rows and V^T columns: 8 (key, 4-column) pieces per thread per round,
    // all 16 loads in flight before the first LDS store
    for (int base = 0; base < Np * (KLD / 4); base += 8 * (int)blockDim.x) {
        uint2 kr[8], vr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + threadIdx.x + u * blockDim.x;
            const int key = i / (KLD / 4), c = i % (KLD / 4);
            const bool ok = key < N && c < hq;
            const bf16* src = qkv + (row0 + key) * 3 * C + h * hd + 4 * c;
            kr[u] = ldz8(src + C, ok);
            vr[u] = ldz8(src + 2 * C, ok);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + threadIdx.x + u * blockDim.x;
            if (i >= Np * (KLD / 4)) continue;
            const int key = i / (KLD / 4), c = i % (KLD / 4);
            *reinterpret_cast<uint2*>(Ks + key * KLD + 4 * c) = kr[u];
            if (c < hq) {
                const bf16* vb = reinterpret_cast<const bf16*>(&vr[u]);
#pragma unroll
                for (int e = 0; e < 4; ++e) Vt[(4 * c + e) * VLD + key] = vb[e];
            }
        }
    }
    for (int i = threadIdx.x; i < VLD; i += blockDim.x) Vt[hd * VLD + i] = (bf16)0.0f;
    for (int i = threadIdx.x; i < hd * (VLD - Np); i += blockDim.x)
        Vt[(i / (VLD - Np)) * VLD + Np + i % (VLD - Np)] = (bf16)0.0f;
    stage_bias(bias_s, nullptr, a.table, a.nrel, a.heads, h);
    for (int i = threadIdx.x; i < Np; i += blockDim.x) {
        const int lb = ldzi(a.labels + row0 + i, a.labels != nullptr && i < N);
        lab_s[i] = i < N ? (rel_term(i, a) << 5) | lb : 0;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int hh = lane >> 5;
    const int nqb = Np / 32, nkb = Np / 32;
    const int c0 = rel_c0(a);
    for (int qb = blockIdx.y * nw + wave; qb < nqb; qb += gridDim.y * nw) {
        const int q = qb * 32 + (lane & 31);
        const bool qvalid = q < N;
        // Q fragments (B operand of S^T = K Q^T), scaled (vst:149)
        Frag8<bf16> qf[2];
        head_frags(qf, qkv, 3 * C, row0 + q, h * hd, qvalid, hd, hh, a.scale);
        const int qinfo = qvalid ? lab_s[q] : 0;
        const int fq = (qinfo >> 5) + c0;
        const int dl = min(lane & 31, hd);          // V^T row of this lane (row hd is zero)
        float m = -INFINITY, l = 0.0f;
        f32x16 z = (f32x16)0.0f;                    // O^T: rows d, cols q (lane)
        for (int kb = 0; kb < nkb; ++kb) {
            f32x16 s = (f32x16)0.0f;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const Frag8<bf16> kf = load8<bf16>(Ks + (kb * 32 + (lane & 31)) * KLD + kk * 16 + 8 * hh);
                mfma32(s, kf, qf[kk]);
            }
            // branch-free element phase: all 16 label / bias LDS reads issued
            // before use; padded keys / queries read in-range entries (lab_s
            // holds Np entries, the bias index is clamped) and become -inf
            int kinfo[16];
            float bv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) kinfo[r] = lab_s[kb * 32 + acc_row(r, lane)];
#pragma unroll
            for (int r = 0; r < 16; ++r) bv[r] = bias_s[min(max(fq - (kinfo[r] >> 5), 0), a.nrel - 1)];
            float tm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kb * 32 + acc_row(r, lane);
                const float v = s[r] + bv[r] + mask_term<MM>(a, w, min(q, N - 1), min(key, N - 1), qinfo, kinfo[r]);
                s[r] = (key < N && qvalid) ? v : -INFINITY;
                tm = fmaxf(tm, s[r]);
            }
            tm = xor32_max(tm);
            const float mn = fmaxf(m, tm);
            // no branch: every lane reaches the MFMAs (a query with nothing valid
            // yet uses reference 0: alpha = exp(-inf) = 0, p = exp(-inf) = 0)
            const float mref = (mn == -INFINITY) ? 0.0f : mn;
            const float alpha = __expf(m - mref);
            m = mn;
            l *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] *= alpha;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                Frag8<bf16> pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float pv = __expf(s[8 * st + j] - mref);
                    l += pv;
                    pf.v[j] = (bf16)pv;
                }
                const bf16* vrow = Vt + dl * VLD + kb * 32 + 16 * st + 4 * hh;
                const Frag8<bf16> vf = load4x2<bf16>(vrow, vrow + 8);
                mfma32(z, vf, pf);                  // O^T += V^T P^T
            }
        }
        l = xor32_sum(l);
        const float inv_l = (l > 0.0f) ? 1.0f / l : 0.0f;
        // write O: lane = query, registers = d (4 consecutive d per register group)
        if (qvalid) {
            bf16* out = reinterpret_cast<bf16*>(a.out) + (row0 + q) * C + h * hd;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d0 = 8 * g + 4 * hh;
                if (d0 + 3 < hd) {
                    bf16 o4[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) o4[e] = (bf16)(z[4 * g + e] * inv_l);
                    *reinterpret_cast<uint2*>(out + d0) = *reinterpret_cast<const uint2*>(o4);
                }
            }
            if (hh == 0) a.lse[((long)w * a.heads + h) * N + q] = (m == -INFINITY) ? 0.0f : m + __logf(l);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(AttnCfg<T>::BWD_WAVES * 64) attn_bwd_kernel(AttnArgs a) {
    constexpr int KLD = AttnCfg<T>::KLD;
    constexpr int WV = AttnCfg<T>::BWD_WAVES;
    constexpr int NK = WV * 32;               // keys per workgroup
    constexpr int QLD = 32 + 8;               // transposed query tiles
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int N = a.N, hd = a.hd, C = a.heads * a.hd;
    const int Np = (N + 31) & ~31;
    const int KTLD = NK + 8;
    T* Ks = reinterpret_cast<T*>(smem_raw);              // [NK][KLD]
    T* Vs = Ks + NK * KLD;                                 // [NK][KLD]
    T* Kt = Vs + NK * KLD;                                 // [hd+1][KTLD]
    T* Qs = Kt + (hd + 1) * KTLD;                          // [32][KLD]   (scaled q)
    T* dOs = Qs + 32 * KLD;                                // [32][KLD]
    T* Qt = dOs + 32 * KLD;                                // [hd+1][QLD] (scaled q)
    T* dOt = Qt + (hd + 1) * QLD;                          // [hd+1][QLD]
    T* dSs = dOt + (hd + 1) * QLD;                         // [WV][32][KLD]
    float* fb = reinterpret_cast<float*>(dSs + WV * 32 * KLD);
    float* bias_s = fb;                                    // [nrel]
    float* gbias_s = bias_s + a.nrel;                      // [nrel] table-gradient partials of the workgroup
    float* lse_s = gbias_s + a.nrel;                       // [32]
    float* D_s = lse_s + 32;                               // [32]
    float* dQs = D_s + 32;                                 // [WV][32][33] per-wave dQ partials (no atomics)
    float* bins_s = dQs + WV * 32 * 33;                    // [WV][2][kBins] per-wave, per-half local bins
    int* lab_s = reinterpret_cast<int*>(bins_s + WV * 2 * kBins);   // [Np]
    int* brange_s = lab_s + Np;                            // [Np/32][2] rel-term range of each 32-token block

    const int w = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const int key0 = blockIdx.y * NK;
    const T* qkv = reinterpret_cast<const T*>(a.qkv);
    const T* O = reinterpret_cast<const T*>(a.o);
    const T* dO = reinterpret_cast<const T*>(a.dout);
    const long row0 = (long)w * N;

    // hd % 4 == 0 (checked by the host): 4-element vector loads
    const int hq = hd / 4;
    for (int i = threadIdx.x; i < NK * (KLD / 4); i += blockDim.x) {
        const int kl = i / (KLD / 4), c = i % (KLD / 4), key = key0 + kl;
        float kv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, vv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (key < N && c < hq) {
            load4f(qkv + (row0 + key) * 3 * C + C + h * hd + 4 * c, kv);
            load4f(qkv + (row0 + key) * 3 * C + 2 * C + h * hd + 4 * c, vv);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Ks[kl * KLD + 4 * c + e] = from_f<T>(kv[e]);
            Vs[kl * KLD + 4 * c + e] = from_f<T>(vv[e]);
            if (c < hq) Kt[(4 * c + e) * KTLD + kl] = from_f<T>(kv[e]);
        }
    }
    for (int i = threadIdx.x; i < KTLD; i += blockDim.x) Kt[hd * KTLD + i] = from_f<T>(0.0f);
    for (int i = threadIdx.x; i < hd * (KTLD - NK); i += blockDim.x)
        Kt[(i / (KTLD - NK)) * KTLD + NK + i % (KTLD - NK)] = from_f<T>(0.0f);
    stage_bias(bias_s, gbias_s, a.table, a.nrel, a.heads, h);
    for (int i = threadIdx.x; i < WV * 2 * kBins; i += blockDim.x) bins_s[i] = 0.0f;
    for (int i = threadIdx.x; i < Np; i += blockDim.x)
        lab_s[i] = i < N ? (rel_term(i, a) << 5) | (a.labels ? a.labels[row0 + i] : 0) : 0;
    for (int i = threadIdx.x; i < WV * 32 * 33; i += blockDim.x) dQs[i] = 0.0f;
    const int c0 = rel_c0(a);
    for (int bk = threadIdx.x; bk < Np / 32; bk += blockDim.x) {
        int flo = 1 << 30, fhi = -(1 << 30);
        for (int t = bk * 32; t < min(N, bk * 32 + 32); ++t) {
            const int f = rel_term(t, a);
            flo = min(flo, f);
            fhi = max(fhi, f);
        }
        brange_s[2 * bk] = flo;
        brange_s[2 * bk + 1] = fhi;
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5;
    const int kb = wave;                                    // local key block
    const int keyc = key0 + kb * 32 + (lane & 31);          // key on this lane (S layout column)
    const bool kbvalid = key0 + kb * 32 < N;
    f32x16 dv = (f32x16)0.0f, dk = (f32x16)0.0f;
    const int nqb = Np / 32;

    for (int qb = 0; qb < nqb; ++qb) {
        __syncthreads();
        // stage the query block: scaled q, dO, their transposes, lse, D = rowsum(dO * O)
        for (int i = threadIdx.x; i < 32 * (KLD / 4); i += blockDim.x) {
            const int ql = i / (KLD / 4), c = i % (KLD / 4), q = qb * 32 + ql;
            float qv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (q < N && c < hq) {
                load4f(qkv + (row0 + q) * 3 * C + h * hd + 4 * c, qv);
                load4f(dO + (row0 + q) * C + h * hd + 4 * c, gv);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const T qs = from_f<T>(qv[e] * a.scale), gs = from_f<T>(gv[e]);
                Qs[ql * KLD + 4 * c + e] = qs;
                dOs[ql * KLD + 4 * c + e] = gs;
                if (c < hq) { Qt[(4 * c + e) * QLD + ql] = qs; dOt[(4 * c + e) * QLD + ql] = gs; }
            }
        }
        for (int i = threadIdx.x; i < QLD; i += blockDim.x) { Qt[hd * QLD + i] = from_f<T>(0.0f); dOt[hd * QLD + i] = from_f<T>(0.0f); }
        if (threadIdx.x < 32) {
            const int q = qb * 32 + threadIdx.x;
            float dsum = 0.0f, ls = 0.0f;
            if (q < N) {
                for (int c = 0; c < hq; ++c) {
                    float gv[4], ov[4];
                    load4f(dO + (row0 + q) * C + h * hd + 4 * c, gv);
                    load4f(O + (row0 + q) * C + h * hd + 4 * c, ov);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dsum += gv[e] * ov[e];
                }
                ls = a.lse[((long)w * a.heads + h) * N + q];
            }
            D_s[threadIdx.x] = dsum;
            lse_s[threadIdx.x] = ls;
        }
        __syncthreads();
        if (kbvalid) {
            // S and dP tiles, S layout: rows = queries (registers), cols = keys (lanes)
            f32x16 s = (f32x16)0.0f, dp = (f32x16)0.0f;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int kof = kk * 16 + 8 * hh;
                const Frag8<T> qa = load8<T>(Qs + (lane & 31) * KLD + kof);
                const Frag8<T> kbf = load8<T>(Ks + (kb * 32 + (lane & 31)) * KLD + kof);
                mfma32(s, qa, kbf);
                const Frag8<T> ga = load8<T>(dOs + (lane & 31) * KLD + kof);
                const Frag8<T> vbf = load8<T>(Vs + (kb * 32 + (lane & 31)) * KLD + kof);
                mfma32(dp, ga, vbf);
            }
            const int kinfo = lab_s[keyc < Np ? keyc : 0];
            const int klab = kinfo & 31, fk = c0 - (kinfo >> 5);
            // table gradient: the tile's (query, key) pairs fall into rel indices
            // [lo, lo + span); accumulate them in this wave-half's local bins with
            // plain LDS read-add-write (a register's 32 keys hit distinct bins and a
            // wave's LDS ops complete in order), flush once per tile
            const int kblk = (key0 >> 5) + kb;
            const int fq_lo = brange_s[2 * qb], fq_hi = brange_s[2 * qb + 1];
            const int fk_lo = brange_s[2 * kblk], fk_hi = brange_s[2 * kblk + 1];
            const int lo = fq_lo - fk_hi + c0, span = (fq_hi - fq_lo) + (fk_hi - fk_lo) + 1;
            const bool local = span <= kBins;
            float* myb = bins_s + (wave * 2 + hh) * kBins;
            float p[16], ds[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ql = acc_row(r, lane), q = qb * 32 + ql;
                if (q < N && keyc < N) {
                    const int qinfo = lab_s[q];
                    const int ri = (qinfo >> 5) + fk;
                    float v = s[r] + bias_s[ri];
                    if (a.labels && (qinfo & 31) != klab) v += -100.0f;
                    if (a.mask) v += a.mask[((long)(w % a.mask_nw) * N + q) * N + keyc];
                    p[r] = __expf(v - lse_s[ql]);
                    ds[r] = p[r] * (dp[r] - D_s[ql]);
                    if (local) myb[ri - lo] += ds[r];
                    else atomicAdd(gbias_s + ri, ds[r]);
                } else {
                    p[r] = 0.0f;
                    ds[r] = 0.0f;
                }
            }
            if (local) {
                for (int b = lane; b < span; b += 64) {
                    const float g = bins_s[(wave * 2) * kBins + b] + bins_s[(wave * 2 + 1) * kBins + b];
                    bins_s[(wave * 2) * kBins + b] = 0.0f;
                    bins_s[(wave * 2 + 1) * kBins + b] = 0.0f;
                    if (g != 0.0f) atomicAdd(gbias_s + lo + b, g);
                }
            }
            // dV += P^T dO ; dK += dS^T (scale q)   (Z = X^T B, X in the S layout)
            const int d = min(lane & 31, hd);
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                Frag8<T> pf, sf;
#pragma unroll
                for (int j = 0; j < 8; ++j) { pf.v[j] = from_f<T>(p[8 * st + j]); sf.v[j] = from_f<T>(ds[8 * st + j]); }
                const T* go = dOt + d * QLD + 16 * st + 4 * hh;
                mfma32(dv, pf, load4x2<T>(go, go + 8));
                const T* qo = Qt + d * QLD + 16 * st + 4 * hh;
                mfma32(dk, sf, load4x2<T>(qo, qo + 8));
            }
            // dQ = dS K: transpose dS through this wave's LDS scratch
            T* dsw = dSs + wave * 32 * KLD;
#pragma unroll
            for (int r = 0; r < 16; ++r) dsw[acc_row(r, lane) * KLD + (lane & 31)] = from_f<T>(ds[r]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            f32x16 dq = (f32x16)0.0f;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const Frag8<T> af = load8<T>(dsw + (lane & 31) * KLD + kk * 16 + 8 * hh);
                const Frag8<T> bfr = load8<T>(Kt + d * KTLD + kb * 32 + kk * 16 + 8 * hh);
                mfma32(dq, af, bfr);
            }
            if ((lane & 31) < hd) {
#pragma unroll
                for (int r = 0; r < 16; ++r) dQs[(wave * 32 + acc_row(r, lane)) * 33 + (lane & 31)] = dq[r];
            }
        }
        __syncthreads();
        // flush dQ of this query block (scale: dS/dq = scale k)
        for (int i = threadIdx.x; i < 32 * 32; i += blockDim.x) {
            const int ql = i / 32, d = i % 32, q = qb * 32 + ql;
            if (q < N && d < hd) {
                float sum = 0.0f;
#pragma unroll
                for (int wv = 0; wv < WV; ++wv) sum += dQs[(wv * 32 + ql) * 33 + d];
                atomicAdd(a.dqkv + (row0 + q) * 3 * C + h * hd + d, sum * a.scale);
            }
        }
    }
    // dK, dV (rows = keys in registers, cols = d on lanes)
    if (kbvalid && (lane & 31) < hd) {
        const int d = lane & 31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = key0 + kb * 32 + acc_row(r, lane);
            if (key < N) {
                a.dqkv[(row0 + key) * 3 * C + C + h * hd + d] = dk[r];
                a.dqkv[(row0 + key) * 3 * C + 2 * C + h * hd + d] = dv[r];
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.nrel; i += blockDim.x) {
        const float g = gbias_s[i];
        if (g != 0.0f) atomicAdd(a.dtable + i * a.heads + h, g);
    }
}

// ---------------------------------------------------------------- backward, split (bf16)
// Two kernels instead of one, so that no output needs a sum across waves or
// workgroups (no dQ reduction in LDS, no dQ / dK / dV atomics):
//   attn_bwd_kv_kernel : one wave per 32-key block  -> dK, dV, table gradient
//   attn_bwd_q_kernel  : one wave per 32-query block -> dQ
// Each recomputes S and dP for its tiles (P from the forward's log-sum-exp).
// The whole head's operands of the swept side live in LDS as [token][40] bf16
// images (80-B rows: conflict-free ds_read_b128 row reads for the S / dP
// products); the transposed operands of dV^T += dO^T P, dK^T += (sQ)^T dS and
// dQ^T += K^T dS^T are read from the same images with ds_read_b64_tr_b16.  The
// products take their B operand straight from the S / dP accumulators (key on
// the lane in the kv kernel, query on the lane in the q kernel), in the row
// order of the accumulator, so the A operand's two 4-row tr-reads are rows
// {16 st + 4 hh + 0..3} and {+8} of the 32-row tile.
typedef short attn_v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) attn_v4s attn_lds_v4s;
constexpr int kALD = 40;       // LDS row of a [token][d <= 32] image (bf16)
constexpr int kBwdWaves = 7;   // 7 waves x 32 tokens per workgroup; 2 workgroups cover N = 448

// img[t][0..kALD) = sc * src[(row0 + t) * ld + col0 + d] for d < hd, 0 otherwise; t < Np.
// 8-B pieces (4 d), loaded 8 per thread before any is stored, so a workgroup
// pays a few memory latencies for a head, not one per piece.
DLCS_DEV void stage_head(bf16* img, const bf16* src, long ld, long row0, int col0, int N, int Np, int hd, float sc) {
    constexpr int PR = kALD / 4;                   // pieces per image row
    const int hq = hd / 4, total = Np * PR;
    for (int base = 0; base < total; base += 8 * (int)blockDim.x) {
        uint2 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + threadIdx.x + k * blockDim.x;
            const int t = i / PR, c = i % PR;
            v[k] = ldz8(src + (row0 + t) * ld + col0 + 4 * c, i < total && t < N && c < hq);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + threadIdx.x + k * blockDim.x;
            if (i >= total) continue;
            uint2 o = v[k];
            if (sc != 1.0f) {
                const bf16* b = reinterpret_cast<const bf16*>(&v[k]);
                bf16 r[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = (bf16)((float)b[e] * sc);
                o = *reinterpret_cast<const uint2*>(r);
            }
            *reinterpret_cast<uint2*>(img + i * 4) = o;       // i = t * PR + c  ->  t * kALD + 4 c
        }
    }
}

// D[t] = sum_d dO[t][d] * O[t][d] (bf16 operands as stored) for t < Np, from the
// staged dO image and the global O rows
DLCS_DEV void stage_rowdot(float* D, const bf16* Gimg, const bf16* O, long ld, long row0, int col0, int N, int Np, int hd) {
    for (int t = threadIdx.x; t < Np; t += blockDim.x) {
        uint2 o[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            o[c] = ldz8(O + (row0 + t) * ld + col0 + 4 * c, t < N && c < hd / 4);
        }
        float dsum = 0.0f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bf16* ob = reinterpret_cast<const bf16*>(&o[c]);
#pragma unroll
            for (int e = 0; e < 4; ++e) dsum += (float)Gimg[t * kALD + 4 * c + e] * (float)ob[e];
        }
        D[t] = dsum;
    }
}

// A operand of a 32x32x16 MFMA whose rows are the image COLUMNS (d = lane & 31)
// and whose 16 k-slots are the image rows {r0 + 4 hh + 0..3, r0 + 8 + 4 hh + 0..3}
DLCS_DEV Frag8<bf16> tr_operand(const bf16* img, int r0, int lane) {
    const int g = lane >> 4;
    const bf16* p = img + (r0 + 4 * (g >> 1) + ((lane >> 2) & 3)) * kALD + 16 * (g & 1) + (lane & 3) * 4;
    const attn_v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((attn_lds_v4s*)(const_cast<bf16*>(p)));
    const attn_v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((attn_lds_v4s*)(const_cast<bf16*>(p + 8 * kALD)));
    typedef short v8s __attribute__((ext_vector_type(8)));
    const v8s both = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    Frag8<bf16> f;
    f.v = __builtin_bit_cast(bf16x8, both);
    return f;
}


// 16 fp32 accumulator values (rows d = acc_row(r), one token per lane) -> dst[d], d < hd, as float4 stores
DLCS_DEV void store_head_rows(float* dst, const f32x16& acc, int hd, int hh, float sc) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const int d0 = 8 * gq + 4 * hh;
        if (d0 + 3 < hd)
            *reinterpret_cast<float4*>(dst + d0) =
                make_float4(sc * acc[4 * gq], sc * acc[4 * gq + 1], sc * acc[4 * gq + 2], sc * acc[4 * gq + 3]);
    }
}

// Mask mode of a launch: 0 none, 1 shift-region labels (-100 where the labels
// differ, vst:342-355), 2 explicit additive mask [mask_nw, N, N] (vst:157-160).
// Compile-time, so the score loop is branch-free: out-of-range tokens read
// in-range LDS entries and are zeroed by a select.

template <int MM>
__global__ void __launch_bounds__(kBwdWaves * 64) attn_bwd_kv_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int N = a.N, hd = a.hd, C = a.heads * a.hd;
    const int Np = (N + 31) & ~31;
    bf16* Qs = reinterpret_cast<bf16*>(smem_raw);                  // [Np][kALD] scale * q
    bf16* Gs = Qs + Np * kALD;                                      // [Np][kALD] dO
    float* bias_s = reinterpret_cast<float*>(Gs + Np * kALD);      // [nrel] table column of head h
    float* gbias_s = bias_s + a.nrel;                               // [nrel] table gradient of the workgroup
    float* lse_s = gbias_s + a.nrel;                                // [Np]
    float* D_s = lse_s + Np;                                        // [Np] rowsum(dO * O)
    float* bins_s = D_s + Np;                                       // [kBwdWaves][2][kBins + 1] per wave-half bins
    int* lab_s = reinterpret_cast<int*>(bins_s + kBwdWaves * 2 * (kBins + 1));   // [Np] rel term << 5 | region label
    int* brange_s = lab_s + Np;                                     // [Np / 32][2] rel-term range of a 32-token block

    const int w = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const long row0 = (long)w * N;
    const bf16* qkv = reinterpret_cast<const bf16*>(a.qkv);
    const bf16* O = reinterpret_cast<const bf16*>(a.o);
    const bf16* dO = reinterpret_cast<const bf16*>(a.dout);
    stage_head(Qs, qkv, 3 * C, row0, h * hd, N, Np, hd, a.scale);
    stage_head(Gs, dO, C, row0, h * hd, N, Np, hd, 1.0f);
    stage_bias(bias_s, gbias_s, a.table, a.nrel, a.heads, h);
    for (int i = threadIdx.x; i < kBwdWaves * 2 * (kBins + 1); i += blockDim.x) bins_s[i] = 0.0f;
    for (int t = threadIdx.x; t < Np; t += blockDim.x) {
        lse_s[t] = ldzf(a.lse + ((long)w * a.heads + h) * N + t, t < N);
        const int lb = MM == 1 ? ldzi(a.labels + row0 + t, t < N) : 0;
        lab_s[t] = t < N ? (rel_term(t, a) << 5) | lb : 0;
    }
    for (int bk = threadIdx.x; bk < Np / 32; bk += blockDim.x) {
        int lo = 1 << 30, hi = -(1 << 30);
        for (int t = bk * 32; t < min(N, bk * 32 + 32); ++t) { const int f = rel_term(t, a); lo = min(lo, f); hi = max(hi, f); }
        brange_s[2 * bk] = lo;
        brange_s[2 * bk + 1] = hi;
    }
    __syncthreads();
    stage_rowdot(D_s, Gs, O, C, row0, h * hd, N, Np, hd);
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5;
    const int kb = blockIdx.y * kBwdWaves + wave;
    if (kb * 32 < N) {
        const int key = kb * 32 + (lane & 31);
        const bool kvalid = key < N;
        Frag8<bf16> kf[2], vf[2];
        head_frags(kf, qkv, 3 * C, row0 + key, C + h * hd, kvalid, hd, hh, 1.0f);
        head_frags(vf, qkv, 3 * C, row0 + key, 2 * C + h * hd, kvalid, hd, hh, 1.0f);
        const int c0 = rel_c0(a);
        const int kinfo = lab_s[kvalid ? key : 0];
        const int fk = c0 - (kinfo >> 5);
        const int fk_lo = brange_s[2 * kb], fk_hi = brange_s[2 * kb + 1];
        float* myb = bins_s + (wave * 2 + hh) * (kBins + 1);       // slot kBins: discard bin of invalid pairs
        f32x16 dk = (f32x16)0.0f, dv = (f32x16)0.0f;       // dK^T, dV^T: rows d, cols key
        for (int qb = 0; qb < Np / 32; ++qb) {
            // S = (sQ) K^T and dP = dO V^T: rows query (registers), cols key (lane)
            f32x16 s = (f32x16)0.0f, dp = (f32x16)0.0f;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const int off = (qb * 32 + (lane & 31)) * kALD + 16 * st + 8 * hh;
                mfma32(s, load8<bf16>(Qs + off), kf[st]);
                mfma32(dp, load8<bf16>(Gs + off), vf[st]);
            }
            // element phase, branch-free and in three independent batches (row
            // info, bias gather, arithmetic) so the LDS latencies overlap;
            // out-of-range pairs read in-range entries and are zeroed by okf
            float p[16], ds[16];
            int ri[16], qi[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) qi[r] = lab_s[qb * 32 + acc_row(r, lane)];
            float bv[16], lv[16], dv_[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = qb * 32 + acc_row(r, lane);
                ri[r] = (qi[r] >> 5) + fk;
                bv[r] = bias_s[ri[r]];
                lv[r] = lse_s[q];
                dv_[r] = D_s[q];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = qb * 32 + acc_row(r, lane);
                const float okf = (kvalid && q < N) ? 1.0f : 0.0f;
                const float v = s[r] + bv[r] + mask_term<MM>(a, w, min(q, N - 1), min(key, N - 1), qi[r], kinfo);
                p[r] = okf * __expf(v - lv[r]);
                ds[r] = p[r] * (dp[r] - dv_[r]);
            }
            // table gradient: this tile's (query, key) pairs fall into rel indices
            // [lo, lo + span); per wave-half private bins, read-add-write batched
            // (a register's 32 keys hit 32 distinct bins, a lane's 16 queries 16)
            const int lo = brange_s[2 * qb] - fk_hi + c0;
            const int span = brange_s[2 * qb + 1] - brange_s[2 * qb] + fk_hi - fk_lo + 1;
            if (span <= kBins) {
                // one register = 32 distinct bins per half, so each register's
                // read-add-write is race-free; registers go in order (two lanes
                // of one half can meet in a bin through different registers)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int bi = (kvalid && qb * 32 + acc_row(r, lane) < N) ? ri[r] - lo : kBins;
                    myb[bi] += ds[r];            // (LDS float atomics measured 2.8x slower here)
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (int b = lane; b < span; b += 64) {
                    float* b0 = bins_s + (wave * 2) * (kBins + 1) + b;
                    const float g = b0[0] + b0[kBins + 1];
                    b0[0] = 0.0f;
                    b0[kBins + 1] = 0.0f;
                    if (g != 0.0f) atomicAdd(gbias_s + lo + b, g);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (ds[r] != 0.0f) atomicAdd(gbias_s + ri[r], ds[r]);
            }
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                Frag8<bf16> pf, sf;
#pragma unroll
                for (int j = 0; j < 8; ++j) { pf.v[j] = (bf16)p[8 * st + j]; sf.v[j] = (bf16)ds[8 * st + j]; }
                mfma32(dv, tr_operand(Gs, qb * 32 + 16 * st, lane), pf);    // dV^T += dO^T P
                mfma32(dk, tr_operand(Qs, qb * 32 + 16 * st, lane), sf);    // dK^T += (sQ)^T dS
            }
        }
        if (kvalid) {
            store_head_rows(a.dqkv + (row0 + key) * 3 * C + C + h * hd, dk, hd, hh, 1.0f);
            store_head_rows(a.dqkv + (row0 + key) * 3 * C + 2 * C + h * hd, dv, hd, hh, 1.0f);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.nrel; i += blockDim.x) {
        const float g = gbias_s[i];
        if (g != 0.0f) atomicAdd(a.dtable + i * a.heads + h, g);
    }
}

template <int MM>
__global__ void __launch_bounds__(kBwdWaves * 64) attn_bwd_q_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int N = a.N, hd = a.hd, C = a.heads * a.hd;
    const int Np = (N + 31) & ~31;
    bf16* Ks = reinterpret_cast<bf16*>(smem_raw);                  // [Np][kALD] k
    bf16* Vs = Ks + Np * kALD;                                      // [Np][kALD] v
    float* bias_s = reinterpret_cast<float*>(Vs + Np * kALD);      // [nrel]
    int* lab_s = reinterpret_cast<int*>(bias_s + a.nrel);          // [Np]

    const int w = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const long row0 = (long)w * N;
    const bf16* qkv = reinterpret_cast<const bf16*>(a.qkv);
    const bf16* O = reinterpret_cast<const bf16*>(a.o);
    const bf16* dO = reinterpret_cast<const bf16*>(a.dout);
    stage_head(Ks, qkv, 3 * C, row0, C + h * hd, N, Np, hd, 1.0f);
    stage_head(Vs, qkv, 3 * C, row0, 2 * C + h * hd, N, Np, hd, 1.0f);
    stage_bias(bias_s, nullptr, a.table, a.nrel, a.heads, h);
    for (int t = threadIdx.x; t < Np; t += blockDim.x) {
        const int lb = MM == 1 ? ldzi(a.labels + row0 + t, t < N) : 0;
        lab_s[t] = t < N ? (rel_term(t, a) << 5) | lb : 0;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5;
    const int qb = blockIdx.y * kBwdWaves + wave;
    if (qb * 32 >= N) return;
    const int q = qb * 32 + (lane & 31);
    const bool qvalid = q < N;
    Frag8<bf16> qf[2], gf[2];
    head_frags(qf, qkv, 3 * C, row0 + q, h * hd, qvalid, hd, hh, a.scale);
    head_frags(gf, dO, C, row0 + q, h * hd, qvalid, hd, hh, 1.0f);
    float D = 0.0f;
    {
        uint2 g8[8], o8[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool ok = qvalid && c < hd / 4;
            g8[c] = ldz8(dO + (row0 + q) * C + h * hd + 4 * c, ok);
            o8[c] = ldz8(O + (row0 + q) * C + h * hd + 4 * c, ok);
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bf16* gb = reinterpret_cast<const bf16*>(&g8[c]);
            const bf16* ob = reinterpret_cast<const bf16*>(&o8[c]);
#pragma unroll
            for (int e = 0; e < 4; ++e) D += (float)gb[e] * (float)ob[e];
        }
    }
    const float lse = ldzf(a.lse + ((long)w * a.heads + h) * N + q, qvalid);
    const int qinfo = lab_s[qvalid ? q : 0];
    const int fq = (qinfo >> 5) + rel_c0(a);
    f32x16 dq = (f32x16)0.0f;                          // dQ^T: rows d, cols query
    for (int kb = 0; kb < Np / 32; ++kb) {
        // S^T = K (sQ)^T and dP^T = V dO^T: rows key (registers), cols query (lane)
        f32x16 s = (f32x16)0.0f, dp = (f32x16)0.0f;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const int off = (kb * 32 + (lane & 31)) * kALD + 16 * st + 8 * hh;
            mfma32(s, load8<bf16>(Ks + off), qf[st]);
            mfma32(dp, load8<bf16>(Vs + off), gf[st]);
        }
        // element phase: branch-free, batched LDS reads (see the kv kernel)
        float ds[16], bv[16];
        int ki[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) ki[r] = lab_s[kb * 32 + acc_row(r, lane)];
#pragma unroll
        for (int r = 0; r < 16; ++r) bv[r] = bias_s[fq - (ki[r] >> 5)];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kb * 32 + acc_row(r, lane);
            const float okf = (qvalid && key < N) ? 1.0f : 0.0f;
            const float v = s[r] + bv[r] + mask_term<MM>(a, w, min(q, N - 1), min(key, N - 1), qinfo, ki[r]);
            ds[r] = okf * __expf(v - lse) * (dp[r] - D);
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            Frag8<bf16> sf;
#pragma unroll
            for (int j = 0; j < 8; ++j) sf.v[j] = (bf16)ds[8 * st + j];
            mfma32(dq, tr_operand(Ks, kb * 32 + 16 * st, lane), sf);      // dQ^T += K^T dS^T
        }
    }
    if (qvalid) store_head_rows(a.dqkv + (row0 + q) * 3 * C + h * hd, dq, hd, hh, a.scale);
}

size_t bwd_kv_smem(const AttnArgs& a) {
    const int Np = (a.N + 31) & ~31;
    return (size_t)2 * Np * kALD * 2 + (size_t)(2 * a.nrel + 3 * Np + kBwdWaves * 2 * (kBins + 1)) * 4 + (size_t)(Np / 32) * 8;
}
size_t bwd_q_smem(const AttnArgs& a) {
    const int Np = (a.N + 31) & ~31;
    return (size_t)2 * Np * kALD * 2 + (size_t)(a.nrel + Np) * 4;
}

template <typename T>
size_t fwd_smem(const AttnArgs& a) {
    const int Np = (a.N + 31) & ~31;
    return (size_t)Np * AttnCfg<T>::KLD * sizeof(T) + (size_t)(a.hd + 1) * (Np + 8) * sizeof(T) +
           (size_t)a.nrel * 4 + (size_t)Np * 4 + 16;
}

template <typename T>
size_t bwd_smem(const AttnArgs& a) {
    constexpr int KLD = AttnCfg<T>::KLD, WV = AttnCfg<T>::BWD_WAVES, NK = WV * 32;
    const int Np = (a.N + 31) & ~31;
    size_t t = (size_t)2 * NK * KLD + (size_t)(a.hd + 1) * (NK + 8) + 2 * 32 * KLD + 2 * (a.hd + 1) * 40 +
               (size_t)WV * 32 * KLD;
    return t * sizeof(T) + (size_t)(2 * a.nrel + 64 + WV * 32 * 33 + WV * 2 * kBins) * 4 + (size_t)Np * 4 +
           (size_t)(Np / 32) * 8 + 16;
}

#include "attention_f32.inc"
#include "attention_h3.inc"
#include "mhsa_h3.inc"

bool attn_f32_generic() {
    static const bool g = [] { const char* e = dlcs_knob("DLCS_ATTN_F32_GENERIC"); return e && *e == '1'; }();
    return g;
}
// fp32 forward / backward on the f16 split (attention_h3.inc); DLCS_ATTN_H3=0 keeps
// both on the f32-MFMA kernels, DLCS_ATTN_H3_BWD=0 only the backward
bool attn_fwd_h3() {
    static const bool g = [] { const char* e = dlcs_knob("DLCS_ATTN_H3"); return !(e && *e == '0'); }();
    return g;
}
// Staging-cost diagnostic, compiled only into a profiling build (make
// DIAG=1 -> -DDLCS_DIAG_NLOOP): DLCS_ATTN_H3_NLOOP=k makes the h3 kernels' main
// loops visit k token blocks (outputs are then wrong by design).  The product
// library always runs every block.
int attn_h3_nloop() {
#ifdef DLCS_DIAG_NLOOP
    static const int n = [] { const char* e = dlcs_knob("DLCS_ATTN_H3_NLOOP"); return e ? atoi(e) : 1 << 20; }();
    return n;
#else
    return 1 << 20;
#endif
}
// DIAG build: DLCS_ATTN_EXP (read per launch) -- bits that skip parts of the h3
// kernels' inner loops to time them (outputs wrong by design); 0 in the product
int attn_exp_bits() {
#ifdef DLCS_DIAG_BUILD
    const char* e = dlcs_knob("DLCS_ATTN_EXP");
    return e ? atoi(e) : 0;
#else
    return 0;
#endif
}
bool attn_bwd_h3() {
    static const bool g = [] { const char* e = dlcs_knob("DLCS_ATTN_H3_BWD"); return attn_fwd_h3() && !(e && *e == '0'); }();
    return g;
}

}  // namespace

// dlcs_mhsa_fwd (dit.hip) on the fp16 split: mhsa_h3.inc
int dlcs_mhsa_fwd_h3_internal(const float* qkv, float* out, float* lse, int nseq, int N, int heads, int hd,
                              float scale, hipStream_t st) {
    MhsaH3Args a{qkv, out, lse, nseq, N, heads, scale};
    return mhsa_fwd_h3_launch(a, hd, st);
}

// dlcs_mhsa_bwd (dit.hip) on the fp16 split after its D = rowsum(dO O) pass: mhsa_h3.inc
int dlcs_mhsa_bwd_h3_internal(const float* qkv, const float* dout, const float* lse, const float* dsum, float* dqkv,
                              int nseq, int N, int heads, int hd, float scale, hipStream_t st) {
    MhsaBwdH3Args a{qkv, dout, lse, dsum, dqkv, nseq, N, heads, scale};
    return mhsa_bwd_h3_launch(a, hd, st);
}

extern "C" {

int dlcs_window_attn_fwd(int dtype, const void* qkv, void* out, float* lse, const float* table,
                         const int32_t* labels, const float* mask, int64_t mask_nw, int64_t nwin, int64_t N, int64_t heads, int64_t head_dim,
                         int64_t wd0, int64_t wh0, int64_t ww0, float scale, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(qkv && out && lse && table && nwin > 0 && N > 0 && heads > 0);
    if (head_dim > 32 || head_dim % 4 || N > 1024 || ((uintptr_t)qkv & 15)) return DLCS_ERR_UNSUPPORTED_SIZE;
    AttnArgs a{};
    a.qkv = qkv; a.out = out; a.lse = lse; a.table = table; a.labels = labels;
    a.mask = mask; a.mask_nw = (int)(mask_nw > 0 ? mask_nw : 1);
    a.nwin = (int)nwin; a.N = (int)N; a.heads = (int)heads; a.hd = (int)head_dim;
    a.nrel = (int)((2 * wd0 - 1) * (2 * wh0 - 1) * (2 * ww0 - 1));
    a.wd0 = (int)wd0; a.wh0 = (int)wh0; a.ww0 = (int)ww0; a.scale = scale;
    a.nloop = attn_h3_nloop();
    a.exp = attn_exp_bits();
    const int nqb = (int)((N + 31) / 32);
    dim3 grid((unsigned)(nwin * heads), cdiv(nqb, FWD_WAVES));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DLCS_F32 && head_dim == 20 && !attn_f32_generic())
    {   // windows whose f16 images exceed the LDS take the f32-MFMA kernel
        if (attn_fwd_h3()) { const int rc = attn_fwd_h3_launch(a, st); if (rc != DLCS_ERR_UNSUPPORTED_SIZE) return rc; }
        return attn_fwd_f32_launch<20>(a, st);
    }
    if (dtype == DLCS_F32) {
        size_t sm = fwd_smem<float>(a);
        if (sm > 160 * 1024) return DLCS_ERR_UNSUPPORTED_SIZE;
        (void)hipFuncSetAttribute((const void*)attn_fwd_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
        hipLaunchKernelGGL(attn_fwd_kernel<float>, grid, dim3(FWD_WAVES * 64), sm, st, a);
    } else {
        size_t sm = fwd_smem<bf16>(a);
        if (sm > 160 * 1024) return DLCS_ERR_UNSUPPORTED_SIZE;
        // single-pass kernel: 2 workgroups per (window, head), ceil(nqb / 2) waves each
        const int waves = std::min(16, (nqb + 1) / 2);
        const int mm = mask ? 2 : (labels ? 1 : 0);
#define ATTN_FWD_LAUNCH(M)                                                                                         \
    (void)hipFuncSetAttribute((const void*)attn_fwd_v2_kernel<M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm); \
    hipLaunchKernelGGL(attn_fwd_v2_kernel<M>, dim3((unsigned)(nwin * heads), 2), dim3(waves * 64), sm, st, a)
        if (mm == 2) { ATTN_FWD_LAUNCH(2); }
        else if (mm == 1) { ATTN_FWD_LAUNCH(1); }
        else { ATTN_FWD_LAUNCH(0); }
#undef ATTN_FWD_LAUNCH
    }
    return dlcs_launch_status();
}

int dlcs_window_attn_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse,
                         const float* table, const int32_t* labels, const float* mask, int64_t mask_nw,
                         float* dqkv, float* dtable,
                         int64_t nwin, int64_t N, int64_t heads, int64_t head_dim,
                         int64_t wd0, int64_t wh0, int64_t ww0, float scale, dlcs_stream_t stream) {
    DLCS_CHECK_ARG(qkv && out && dout && lse && table && dqkv && dtable && nwin > 0 && N > 0 && heads > 0);
    if (head_dim > 32 || head_dim % 4 || N > 1024 || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 15) || ((uintptr_t)dout & 15)) return DLCS_ERR_UNSUPPORTED_SIZE;
    AttnArgs a{};
    a.qkv = qkv; a.o = out; a.dout = dout; a.lse = (float*)lse; a.table = table; a.labels = labels;
    a.mask = mask; a.mask_nw = (int)(mask_nw > 0 ? mask_nw : 1);
    a.dqkv = dqkv; a.dtable = dtable;
    a.nwin = (int)nwin; a.N = (int)N; a.heads = (int)heads; a.hd = (int)head_dim;
    a.nrel = (int)((2 * wd0 - 1) * (2 * wh0 - 1) * (2 * ww0 - 1));
    a.wd0 = (int)wd0; a.wh0 = (int)wh0; a.ww0 = (int)ww0; a.scale = scale;
    a.nloop = attn_h3_nloop();
    a.exp = attn_exp_bits();
    hipStream_t st = (hipStream_t)stream;
    // the fp16-split and bf16 kernels write every element of dqkv; the f32-MFMA kernels
    // accumulate dQ with atomics, so their buffer is zeroed here (the caller never zeroes)
    const size_t dq_bytes = (size_t)nwin * N * 3 * heads * head_dim * sizeof(float);
    if (dtype == DLCS_F32 && head_dim == 20 && !attn_f32_generic())
    {
        if (attn_bwd_h3()) { const int rc = attn_bwd_h3_launch(a, st); if (rc != DLCS_ERR_UNSUPPORTED_SIZE) return rc; }
        // a refused call writes nothing: the size check comes before the memset
        if (bwd_kv_f32_smem<20>(a) > 160 * 1024 || bwd_q_f32_smem<20>(a) > 160 * 1024) return DLCS_ERR_UNSUPPORTED_SIZE;
        if (hipMemsetAsync(dqkv, 0, dq_bytes, st) != hipSuccess) return dlcs_launch_status();
        return attn_bwd_f32_launch<20>(a, st);
    }
    if (dtype == DLCS_F32) {
        constexpr int NK = AttnCfg<float>::BWD_WAVES * 32;
        size_t sm = bwd_smem<float>(a);
        if (sm > 160 * 1024) return DLCS_ERR_UNSUPPORTED_SIZE;
        if (hipMemsetAsync(dqkv, 0, dq_bytes, st) != hipSuccess) return dlcs_launch_status();
        dim3 grid((unsigned)(nwin * heads), cdiv(N, NK));
        (void)hipFuncSetAttribute((const void*)attn_bwd_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
        hipLaunchKernelGGL(attn_bwd_kernel<float>, grid, dim3(AttnCfg<float>::BWD_WAVES * 64), sm, st, a);
    } else {
        // split backward: dK / dV / table gradient (key-owned) and dQ (query-owned)
        const size_t s1 = bwd_kv_smem(a), s2 = bwd_q_smem(a);
        if (s1 > 160 * 1024 || s2 > 160 * 1024) return DLCS_ERR_UNSUPPORTED_SIZE;
        dim3 grid((unsigned)(nwin * heads), cdiv(cdiv(N, 32), kBwdWaves));
        const int mm = a.mask ? 2 : (a.labels ? 1 : 0);
#define ATTN_BWD_LAUNCH(M) do { \
            (void)hipFuncSetAttribute((const void*)attn_bwd_kv_kernel<M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s1); \
            hipLaunchKernelGGL(attn_bwd_kv_kernel<M>, grid, dim3(kBwdWaves * 64), s1, st, a); \
            (void)hipFuncSetAttribute((const void*)attn_bwd_q_kernel<M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s2); \
            hipLaunchKernelGGL(attn_bwd_q_kernel<M>, grid, dim3(kBwdWaves * 64), s2, st, a); } while (0)
        if (mm == 2) ATTN_BWD_LAUNCH(2);
        else if (mm == 1) ATTN_BWD_LAUNCH(1);
        else ATTN_BWD_LAUNCH(0);
#undef ATTN_BWD_LAUNCH
    }
    return dlcs_launch_status();
}

}  // extern "C"
