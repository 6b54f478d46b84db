// Included by sense.hip (inside its anonymous namespace, after sense_fast.inc:
// uses its compile-time ccos_d / csin_d, and FftPlan / FftAux / BlueLds /
// fft_lds / build_twiddles / cmul of sense.hip).
//
// Line lengths that are not 2-3-5-smooth, on the dense generic kernels:
//  * dft_odd<7|11|13>: the in-register butterflies of the extra Stockham passes;
//  * Bluestein's chirp-z for every other length n <= 1024.  With
//    w_k = exp(-+ i pi k^2 / n) (forward / inverse) and jk = (j^2 + k^2 - (k-j)^2) / 2,
//        X_k = w_k * sum_j (x_j w_j) conj(w_{k-j}),
//    a linear convolution, run as a circular one of length m >= 2n - 1 with the
//    block's inner smooth FFT: zero-extend x w to m, FFT_m, times the filter
//    spectrum FFT_m(wrapped conj(w)) / m, IFFT_m, times w, keep n points.
//    Chirp, inner twiddles and filter spectrum are built per block in LDS, once,
//    before its lines (and before the coil loop of the row modes 1 and 2): no
//    device-global table, no allocation, nothing that outlives the call.

struct OddRoots { float c[7]; float s[7]; };
// cos and sin of 2 pi q / R, q <= (R - 1) / 2 <= 6, evaluated at compile time
constexpr OddRoots odd_roots(int R) {
    OddRoots t{};
    for (int q = 0; q <= (R - 1) / 2; ++q) {
        const double x = 2.0 * kPiD * q / R;
        t.c[q] = (float)ccos_d(x);
        t.s[q] = (float)csin_d(x);
    }
    return t;
}

// R-point DFT, R an odd prime: the conjugate pairs a[j] +- a[R-j] are folded, so
// X_k, X_{R-k} = (a0 + sum_j cos(2 pi jk/R) t_j) -+ i (sum_j sin(2 pi jk/R) d_j),
// (R-1)^2 / 2 real multiplies per component pair instead of (R-1)^2.
template <int R>
DLCS_DEV void dft_odd(float2 (&a)[R], bool inv) {
    static_assert(R == 7 || R == 11 || R == 13, "odd radices of the mixed plans");
    constexpr int H = (R - 1) / 2;
    constexpr OddRoots W = odd_roots(R);
    float2 t[H], d[H];
#pragma unroll
    for (int j = 1; j <= H; ++j) {
        t[j - 1] = cadd(a[j], a[R - j]);
        d[j - 1] = csub(a[j], a[R - j]);
    }
    const float2 a0 = a[0];
    float2 s0 = a0;
#pragma unroll
    for (int j = 0; j < H; ++j) s0 = cadd(s0, t[j]);
    a[0] = s0;
#pragma unroll
    for (int k = 1; k <= H; ++k) {
        float2 m = a0, n = make_float2(0.f, 0.f);
#pragma unroll
        for (int j = 1; j <= H; ++j) {
            const int q = (j * k) % R;
            const float c = W.c[q <= H ? q : R - q];
            const float s = q <= H ? W.s[q] : -W.s[R - q];
            m.x += c * t[j - 1].x; m.y += c * t[j - 1].y;
            n.x += s * d[j - 1].x; n.y += s * d[j - 1].y;
        }
        // forward: -i n ; inverse (conjugate roots): +i n
        const float2 r = inv ? make_float2(-n.y, n.x) : make_float2(n.y, -n.x);
        a[k] = cadd(m, r);
        a[R - k] = csub(m, r);
    }
}

// exp(sign * i pi k^2 / n): k^2 reduced mod 2n in integers (k <= 1023), the
// angle in double -- a single-precision k^2 / n loses the phase at n ~ 1000.
DLCS_DEV float2 chirp_at(int k, int n, double sign) {
    double s, c;
    sincospi(sign * (double)((k * k) % (2 * n)) / (double)n, &s, &c);
    return make_float2((float)c, (float)s);
}

// Per-block tables of a GEN 2 kernel; `behind` is the LDS after the staged lines.
// chirp <- w (n points), bl.twm <- twiddles of the inner length m,
// bl.filt <- FFT_m(b) / m with b[j] = b[m - j] = conj(w_j), j < n, zero between.
// Ends on a barrier.
template <int MAXPTS>
DLCS_DEV void blue_tables(float2* chirp, float2* behind, int n, const FftAux& ax, bool inv, BlueLds& bl) {
    const int m = ax.m;
    bl.twm = behind;
    bl.filt = behind + m;
    bl.work = behind + 2 * m;
    const double sign = inv ? 1.0 : -1.0;
    build_twiddles(bl.twm, m);
    for (int k = threadIdx.x; k < n; k += kThreads) chirp[k] = chirp_at(k, n, sign);
    const float rm = 1.0f / (float)m;
    for (int i = threadIdx.x; i < m; i += kThreads) {
        const int j = i < n ? i : m - i;
        float2 b = make_float2(0.f, 0.f);
        if (j < n) {
            b = chirp_at(j, n, -sign);
            b = make_float2(b.x * rm, b.y * rm);
        }
        bl.filt[i] = b;
    }
    __syncthreads();
    fft_lds<MAXPTS, 0>(bl.filt, 1, m, 1, ax.inner, bl.twm, false);
}

// fft_lds for a Bluestein length: `nbatch` length-n lines at buf[i*si + b*sb],
// transformed in place through bl.work (nbatch lines of m points, same
// orientation as buf).  nbatch * m <= MAXPTS * kThreads (blue_lines).
template <int MAXPTS>
DLCS_DEV void bluestein_lds(float2* buf, int si, int sb, int nbatch, int n, const FftAux& ax,
                            const float2* chirp, const BlueLds& bl, bool inv) {
    const int m = ax.m;
    const bool ifast = (si == 1);
    const int wsi = ifast ? 1 : nbatch, wsb = ifast ? m : 1;
    const int total = nbatch * m;
    // work[idx], idx = i*wsi + b*wsb
    for (int idx = threadIdx.x; idx < total; idx += kThreads) {
        const int b = ifast ? idx / m : idx % nbatch;
        const int i = ifast ? idx % m : idx / nbatch;
        bl.work[idx] = i < n ? cmul(buf[i * si + b * sb], chirp[i]) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    // FFT_m, times the filter spectrum, IFFT_m: one copy of the inner passes' code
#pragma nounroll
    for (int back = 0; back < 2; ++back) {
        fft_lds<MAXPTS, 0>(bl.work, wsi, wsb, nbatch, ax.inner, bl.twm, back != 0);
        if (back) break;
        for (int idx = threadIdx.x; idx < total; idx += kThreads) {
            const int i = ifast ? idx % m : idx / nbatch;
            bl.work[idx] = cmul(bl.work[idx], bl.filt[i]);
        }
        __syncthreads();
    }
    for (int idx = threadIdx.x; idx < nbatch * n; idx += kThreads) {
        const int b = ifast ? idx / n : idx % nbatch;
        const int i = ifast ? idx % n : idx / nbatch;
        buf[i * si + b * sb] = cmul(bl.work[i * wsi + b * wsb], chirp[i]);
    }
    __syncthreads();
}

// Dynamic LDS of every configuration stays within the 64 KB a kernel gets
// without opting in: 8192 complex points.
constexpr int kLdsPoints = 65536 / (int)sizeof(float2);

// LDS points of a Bluestein block of `lines` lines: chirp [n], lines [lines*n],
// inner twiddles [m], filter spectrum [m], padded lines [lines*m].
static size_t blue_lds_points(int n, int m, int lines) {
    return (size_t)n + (size_t)lines * n + 2 * (size_t)m + (size_t)lines * m;
}

// Lines per Bluestein block: the padded lines fit the registers of one inner
// pass (maxpoints = MAXPTS * kThreads) and the block fits kLdsPoints.  The worst
// case n = 1023, m = 2048 holds one line in 8190 points.
static int blue_lines(int n, int m, int maxpoints, int cap) {
    int l = std::min(maxpoints / m, (kLdsPoints - 2 * m - n) / (n + m));
    l = std::min(l, cap);
    return l < 1 ? 1 : l;
}
