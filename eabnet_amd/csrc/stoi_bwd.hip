// The gradient kernels of the intelligibility loss (the value's are in stoi.hip; the shared definitions in stoi_common.h).
#include "stoi_common.h"
#include "fft_lds.h"

#define STOI_TILE_STRIDE (STOI_TILE_FRAMES + 4)

// The gradient of loss_b = -(factor_stoi stoi_b + factor_estoi estoi_b) with respect to the processed signal: the
// literal derivative of rules 2-10 with K, kept and T constant (they come from clean alone), zero through a band value that is
// exactly 0, and rule 9's min differentiated on the branch it took (alpha included).  Three launches on the workspace the value
// call left behind (window, twiddles, K, kept and the band values of both signals):
//   B1  stoi_segments_bwd_kernel  16 segments per workgroup, thread (segment, band), from the same LDS tile and the same fp64
//                                 statistics as kernel 4: d loss / d Y[band][m + t] of segment m alone -> part[b][m][band][t], fp64.
//   B2  stoi_bands_bwd_kernel     8 compacted frames of the processed signal per workgroup: gY[band][t] = the <= 30 partials of the
//                                 segments that hold frame t, in ascending segment order; the frame rebuilt and transformed as in
//                                 kernel 3; bins 7..218 scaled by gY / Y; the adjoint of the zero-padded 512-point real transform as
//                                 ONE 256-point complex transform (the Hermitian half-length packing, same passes); times w; the 256
//                                 samples stored to frames[b][t].
//   B3  stoi_gather_bwd_kernel    one sample of the processed signal per thread: the source frames j - 1 and j that hold it (in that
//                                 order), each through the inverse of kept (a binary search) into the at most two compacted frames
//                                 that overlap it (ascending t, fp32 sum), times w by one fmaf each.  Zero where no kept frame
//                                 covers the sample, past the last frame of rule 3, from the signal's own length to the row's end and
//                                 on the whole row when fewer than 30 band frames remain.
// grad_out is read on the device; no atomics; every sum has one order that depends on the utterance alone.
struct StoiBwdWork {              // byte offsets into the gradient's workspace
    size_t part, frames, total;
};

static StoiBwdWork stoi_bwd_layout(int B, int FC) {
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    StoiBwdWork w;
    w.part = 0;
    w.frames = up((size_t)B * FC * STOI_BANDS * STOI_SEG * sizeof(double));
    w.total = up(w.frames + (size_t)B * FC * STOI_N * sizeof(float));
    return w;
}

__global__ __launch_bounds__(STOI_THREADS) void stoi_segments_bwd_kernel(int FC, const int32_t* __restrict__ K,
                                                                         const float* __restrict__ tob,
                                                                         const float* __restrict__ grad_out, int grad_out_stride,
                                                                         double c_stoi, double c_estoi, double* __restrict__ part) {
    __shared__ float tile[2][STOI_BANDS][STOI_TILE_STRIDE];             // frames s0 .. s0 + 44 of both signals
    __shared__ double rowst[STOI_TILE][STOI_BANDS][4];                  // ESTOI rows: mean and 1 / (norm + eps) of x and of y
    __shared__ double colst[STOI_TILE][STOI_SEG][6];                    // columns: see the column pass
    const int tid = threadIdx.x, b = blockIdx.y;
    const int T = K[b] - 1, S = T - (STOI_SEG - 1), s0 = blockIdx.x * STOI_TILE;
    if (S <= 0 || s0 >= S) return;                                      // (workgroup-uniform, before any barrier)
    for (int e = tid; e < 2 * STOI_BANDS * STOI_TILE_FRAMES; e += STOI_THREADS) {
        const int r = e / STOI_TILE_FRAMES, fr = e - r * STOI_TILE_FRAMES;
        const int t = s0 + fr;
        (&tile[0][0][0])[r * STOI_TILE_STRIDE + fr] = t < T ? tob[((size_t)b * 2 * STOI_BANDS + r) * FC + t] : 0.0f;
    }
    __syncthreads();
    const int sl = tid >> 4, i = tid & 15;
    const bool active = i < STOI_BANDS && s0 + sl < S;
    const double inv_n = 1.0 / (double)STOI_SEG, inv_j = 1.0 / (double)STOI_BANDS;
    const double g = (double)grad_out[(size_t)b * grad_out_stride];
    const double cs = -(c_stoi * g) / ((double)STOI_BANDS * (double)S), ce = -(c_estoi * g) / ((double)STOI_SEG * (double)S);
    const double clip = 1.0 + 5.623413251903491;
    const float* xr = &tile[0][i < STOI_BANDS ? i : 0][sl];
    const float* yr = &tile[1][i < STOI_BANDS ? i : 0][sl];
    double mx = 0.0, my = 0.0, rx = 0.0, ry = 0.0, ny = 0.0;            // row statistics (ny = the norm of y - my)
    double alpha = 0.0, mp = 0.0, rp = 0.0, kq = 0.0, mgq = 0.0, ga = 0.0, ca = 0.0;
    if (active) {
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0;
        for (int t = 0; t < STOI_SEG; ++t) {
            const double xv = (double)xr[t], yv = (double)yr[t];
            sx += xv; sy += yv; sxx += xv * xv; syy += yv * yv;
        }
        const double nx2 = sqrt(sxx), ny2 = sqrt(syy);
        alpha = nx2 / (ny2 + STOI_EPS);
        ca = ny2 > 0.0 ? -nx2 / ((ny2 + STOI_EPS) * (ny2 + STOI_EPS)) / ny2 : 0.0;      // d alpha / d y[t] = ca y[t]
        mx = sx * inv_n;
        my = sy * inv_n;
        double sp = 0.0, cxx = 0.0, cyy = 0.0;
        for (int t = 0; t < STOI_SEG; ++t) {
            const double xv = (double)xr[t], yv = (double)yr[t];
            sp += fmin(alpha * yv, clip * xv);
            cxx += (xv - mx) * (xv - mx);
            cyy += (yv - my) * (yv - my);
        }
        mp = sp * inv_n;
        ny = sqrt(cyy);
        rx = 1.0 / (sqrt(cxx) + STOI_EPS);
        ry = 1.0 / (ny + STOI_EPS);
        rowst[sl][i][0] = mx; rowst[sl][i][1] = rx; rowst[sl][i][2] = my; rowst[sl][i][3] = ry;
        if (c_stoi != 0.0) {
            // d = rp sum xn q with q = p - mp, p = min(alpha y, clip x):  d d / d q[t] = rp xn[t] - kq q[t],  kq = (sum xn q) rp^2 / |q|
            double cpp = 0.0, dq = 0.0;
            for (int t = 0; t < STOI_SEG; ++t) {
                const double xv = (double)xr[t], q = fmin(alpha * (double)yr[t], clip * xv) - mp;
                cpp += q * q;
                dq += ((xv - mx) * rx) * q;
            }
            const double np = sqrt(cpp);
            rp = 1.0 / (np + STOI_EPS);
            kq = np > 0.0 ? dq * rp * rp / np : 0.0;
            double sg = 0.0;
            for (int t = 0; t < STOI_SEG; ++t) {
                const double xv = (double)xr[t], q = fmin(alpha * (double)yr[t], clip * xv) - mp;
                sg += rp * ((xv - mx) * rx) - kq * q;
            }
            mgq = sg * inv_n;
            for (int t = 0; t < STOI_SEG; ++t) {                        // d d / d alpha, over the elements on the alpha y branch
                const double xv = (double)xr[t], yv = (double)yr[t];
                if (alpha * yv <= clip * xv) ga += (rp * ((xv - mx) * rx) - kq * (alpha * yv - mp) - mgq) * yv;
            }
        }
    }
    __syncthreads();
    if (active && c_estoi != 0.0) {
        // columns c = i and i + 15 of the row-normalised segment: mean and 1 / (norm + eps) of x and of y, then what the column's
        // normalisation hands back to the rows: g_yc[r] = ce (cy xcn[r] - kc yc[r]),  kc = (sum xcn yc) cy^2 / |yc|,  and its mean
        for (int c = i; c < STOI_SEG; c += STOI_BANDS) {
            double sx = 0.0, sy = 0.0;
            for (int r = 0; r < STOI_BANDS; ++r) {
                sx += ((double)tile[0][r][sl + c] - rowst[sl][r][0]) * rowst[sl][r][1];
                sy += ((double)tile[1][r][sl + c] - rowst[sl][r][2]) * rowst[sl][r][3];
            }
            const double mxc = sx * inv_j, myc = sy * inv_j;
            double cxx = 0.0, cyy = 0.0;
            for (int r = 0; r < STOI_BANDS; ++r) {
                const double xv = ((double)tile[0][r][sl + c] - rowst[sl][r][0]) * rowst[sl][r][1] - mxc;
                const double yv = ((double)tile[1][r][sl + c] - rowst[sl][r][2]) * rowst[sl][r][3] - myc;
                cxx += xv * xv;
                cyy += yv * yv;
            }
            const double nyc = sqrt(cyy);
            const double cx = 1.0 / (sqrt(cxx) + STOI_EPS), cy = 1.0 / (nyc + STOI_EPS);
            double d = 0.0;
            for (int r = 0; r < STOI_BANDS; ++r) {
                const double xv = ((double)tile[0][r][sl + c] - rowst[sl][r][0]) * rowst[sl][r][1] - mxc;
                const double yv = ((double)tile[1][r][sl + c] - rowst[sl][r][2]) * rowst[sl][r][3] - myc;
                d += (xv * cx) * yv;
            }
            const double kc = nyc > 0.0 ? d * cy * cy / nyc : 0.0;
            double sg = 0.0;
            for (int r = 0; r < STOI_BANDS; ++r) {
                const double xv = ((double)tile[0][r][sl + c] - rowst[sl][r][0]) * rowst[sl][r][1] - mxc;
                const double yv = ((double)tile[1][r][sl + c] - rowst[sl][r][2]) * rowst[sl][r][3] - myc;
                sg += cy * (xv * cx) - kc * yv;
            }
            double* o = colst[sl][c];
            o[0] = mxc; o[1] = cx; o[2] = myc; o[3] = cy; o[4] = kc; o[5] = sg * inv_j;
        }
    }
    __syncthreads();
    if (!active) return;                                                // (no barrier below)
    // ESTOI through the row's normalisation: z = y - my, yr = z ry;  g_z[t] = ry g_yr[t] - kr z[t],  kr = (sum g_yr z) ry^2 / |z|
    double kr = 0.0, mgz = 0.0;
    auto g_yr = [&](int t) {
        const double* o = colst[sl][t];
        const double xcn = (((double)xr[t] - mx) * rx - o[0]) * o[1], yc = ((double)yr[t] - my) * ry - o[2];
        return ce * ((o[3] * xcn - o[4] * yc) - o[5]);
    };
    if (c_estoi != 0.0) {
        double a = 0.0;
        for (int t = 0; t < STOI_SEG; ++t) a += g_yr(t) * ((double)yr[t] - my);
        kr = ny > 0.0 ? a * ry * ry / ny : 0.0;
        double sg = 0.0;
        for (int t = 0; t < STOI_SEG; ++t) sg += ry * g_yr(t) - kr * ((double)yr[t] - my);
        mgz = sg * inv_n;
    }
    double* o = part + (((size_t)b * FC + s0 + sl) * STOI_BANDS + i) * STOI_SEG;
    for (int t = 0; t < STOI_SEG; ++t) {
        const double xv = (double)xr[t], yv = (double)yr[t];
        double v = 0.0;
        if (c_stoi != 0.0) {
            double gp = 0.0;
            if (alpha * yv <= clip * xv) gp = (rp * ((xv - mx) * rx) - kq * (alpha * yv - mp) - mgq) * alpha;
            v = cs * (gp + ga * ca * yv);
        }
        if (c_estoi != 0.0) v += (ry * g_yr(t) - kr * (yv - my)) - mgz;
        o[t] = v;
    }
}

__global__ __launch_bounds__(STOI_THREADS) void stoi_bands_bwd_kernel(const StoiRows rows, const int32_t* __restrict__ lens, int FC,
                                                                      const int32_t* __restrict__ kept, const int32_t* __restrict__ K,
                                                                      const float* __restrict__ win_tab,
                                                                      const float2* __restrict__ tw_tab, const float* __restrict__ tob,
                                                                      const double* __restrict__ part, float* __restrict__ frames) {
    __shared__ __attribute__((aligned(16))) float2 tw[2 * STOI_N];
    __shared__ __attribute__((aligned(16))) float2 buf0[FFT_SIGS * STOI_N];
    __shared__ __attribute__((aligned(16))) float2 buf1[FFT_SIGS * STOI_N];
    __shared__ __attribute__((aligned(16))) float win[STOI_N];
    __shared__ float ratio[FFT_SIGS][STOI_BANDS + 1];                   // gY / Y of the workgroup's frames
    __shared__ int src[FFT_SIGS + 2];                                   // kept[t0 - 1 .. t0 + 8], -1 outside [0, K)
    __shared__ unsigned char band_of[STOI_N];                           // the band of a bin in [7, 219)
    const int tid = threadIdx.x, b = blockIdx.y;
    const int Kb = K[b], T = Kb - 1, S = T - (STOI_SEG - 1), t0 = blockIdx.x * FFT_SIGS;
    if (S <= 0 || t0 >= T) return;                                      // (workgroup-uniform, before any barrier)
    int ls, le;
    stoi_lens(lens, rows, b, ls, le);
    const float* x = rows.p[1] + (long long)b * rows.stride[1];
    const bool al = eab_aligned16(x);
    tw[tid] = tw_tab[tid];
    tw[tid + STOI_N] = tw_tab[tid + STOI_N];
    win[tid] = win_tab[tid];
    if (tid < FFT_SIGS + 2) {
        const int t = t0 - 1 + tid;
        src[tid] = (t >= 0 && t < Kb) ? kept[(size_t)b * FC + t] : -1;
    }
    {
        int band = 0;
        while (band < STOI_BANDS - 1 && tid >= stoi_edge[band + 1]) ++band;
        band_of[tid] = (unsigned char)band;
    }
    if (tid < FFT_SIGS * STOI_BANDS) {                                  // frame t lies in the segments max(0, t - 29) .. min(S - 1, t)
        const int f = tid & (FFT_SIGS - 1), band = tid >> 3, t = t0 + f;
        float r = 0.0f;
        if (t < T) {
            double gsum = 0.0;
            const int m_hi = min(S - 1, t);
            for (int m = max(0, t - (STOI_SEG - 1)); m <= m_hi; ++m)
                gsum += part[(((size_t)b * FC + m) * STOI_BANDS + band) * STOI_SEG + (t - m)];
            const float yv = tob[(((size_t)b * 2 + 1) * STOI_BANDS + band) * FC + t];
            if (yv != 0.0f) r = (float)(gsum / (double)yv);
        }
        ratio[f][band] = r;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int f = wave; f < FFT_SIGS; f += STOI_THREADS / 64) {          // the frames of kernel 3, the same way
        const int n = 4 * lane;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t0 + f < T) {                                               // (wave-uniform)
            float own[4], nb[4] = {0.f, 0.f, 0.f, 0.f};
            eab_load4(x, al, STOI_HOP * src[f + 1] + n, le, own);
            const int other = n < STOI_HOP ? src[f] : src[f + 2], on = n < STOI_HOP ? n + STOI_HOP : n - STOI_HOP;
            if (other >= 0) eab_load4(x, al, STOI_HOP * other + on, le, nb);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (win[n + k] * own[k] + win[on + k] * nb[k]) * win[n + k];
        }
        float* z = reinterpret_cast<float*>(buf0) + f * 2 * STOI_N;
        *reinterpret_cast<f32x4*>(z + n) = v;
        *reinterpret_cast<f32x4*>(z + STOI_N + n) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    fft_pass<4>(buf0, buf1, tw, STOI_N, 2 * STOI_N, 256, 1, tid, STOI_THREADS);
    __syncthreads();
    fft_pass<8>(buf1, buf0, tw, STOI_N, 2 * STOI_N, 64, 4, tid, STOI_THREADS);
    __syncthreads();
    fft_pass<8>(buf0, buf1, tw, STOI_N, 2 * STOI_N, 8, 32, tid, STOI_THREADS);
    __syncthreads();
    // H[k] = (gY / Y) X[k] on the bins of the bands, 0 on the others: d loss / d (Re X[k], Im X[k]) as one complex number
    for (int e = tid; e < FFT_SIGS * STOI_N; e += STOI_THREADS) {
        const int f = e >> 8, k = e & (STOI_N - 1);
        float2 h = make_float2(0.0f, 0.0f);
        if (k >= STOI_BIN_LO && k < STOI_BIN_HI) {
            const float2 z = buf1[f * STOI_N + k], zc = buf1[f * STOI_N + STOI_N - k];
            const float2 E = make_float2(0.5f * (z.x + zc.x), 0.5f * (z.y - zc.y));
            const float2 O = make_float2(0.5f * (z.y + zc.y), 0.5f * (zc.x - z.x));
            const float2 wo = cmul(tw[k], O);
            const float r = ratio[f][band_of[k]];
            h = make_float2(r * (E.x + wo.x), r * (E.y + wo.y));
        }
        buf0[e] = h;
    }
    __syncthreads();
    // d loss / d frame[n] = Re sum_k H[k] exp(+2 pi i k n / 512), n < 256.  With k' = (256 - k) mod 256,
    //   C0[k] = (conj H[k] + H[k']) / 2,  C1[k] = W_512^k (conj H[k] - H[k']) / 2
    // are Hermitian, so the 256-point transform of Z = C0 + i C1 is (d[2m], d[2m + 1]) at m.
    for (int e = tid; e < FFT_SIGS * STOI_N; e += STOI_THREADS) {
        const int f = e >> 8, k = e & (STOI_N - 1);
        const float2 h = buf0[e], hc = buf0[f * STOI_N + ((STOI_N - k) & (STOI_N - 1))];
        const float2 c0 = make_float2(0.5f * (h.x + hc.x), 0.5f * (hc.y - h.y));
        const float2 c1 = cmul(tw[k], make_float2(0.5f * (h.x - hc.x), -0.5f * (h.y + hc.y)));
        buf1[e] = make_float2(c0.x - c1.y, c0.y + c1.x);
    }
    __syncthreads();
    fft_pass<4>(buf1, buf0, tw, STOI_N, 2 * STOI_N, 256, 1, tid, STOI_THREADS);
    __syncthreads();
    fft_pass<8>(buf0, buf1, tw, STOI_N, 2 * STOI_N, 64, 4, tid, STOI_THREADS);
    __syncthreads();
    fft_pass<8>(buf1, buf0, tw, STOI_N, 2 * STOI_N, 8, 32, tid, STOI_THREADS);
    __syncthreads();
    for (int e = tid; e < FFT_SIGS * STOI_N; e += STOI_THREADS) {       // times the window of the second framing
        const int f = e >> 8, n = e & (STOI_N - 1);
        if (t0 + f < T)
            frames[((size_t)b * FC + t0 + f) * STOI_N + n] = win[n] * reinterpret_cast<const float*>(buf0)[f * 2 * STOI_N + n];
    }
}

__global__ __launch_bounds__(STOI_THREADS) void stoi_gather_bwd_kernel(const StoiRows rows, const int32_t* __restrict__ lens, int FC,
                                                                       const int32_t* __restrict__ kept, const int32_t* __restrict__ K,
                                                                       const float* __restrict__ win, const float* __restrict__ frames,
                                                                       float* __restrict__ grad, long long grad_stride) {
    const int s = blockIdx.x * STOI_THREADS + threadIdx.x, b = blockIdx.y;
    if (s >= rows.cap[1]) return;
    int ls, le;
    stoi_lens(lens, rows, b, ls, le);
    const int Kb = K[b], T = Kb - 1;
    float g = 0.0f;
    if (T >= STOI_SEG && s < le) {
        const int NF = stoi_frames(max(ls, le));
        const int32_t* kp = kept + (size_t)b * FC;
        const float* fr = frames + (size_t)b * FC * STOI_N;
        for (int h = 1; h >= 0; --h) {                                  // source frame j - 1 (its second half), then j
            const int j = (s >> 7) - h, n = (s & (STOI_HOP - 1)) + STOI_HOP * h;
            if (j < 0 || j >= NF) continue;
            int lo = 0, hi = Kb;                                        // t with kept[t] == j, if any
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (kp[mid] < j) lo = mid + 1; else hi = mid;
            }
            if (lo >= Kb || kp[lo] != j) continue;
            const int t = lo;
            float a = 0.0f;                                             // the compacted frames that overlap the sample, ascending
            if (n < STOI_HOP) {
                if (t >= 1) a += fr[(size_t)(t - 1) * STOI_N + n + STOI_HOP];
                if (t < T) a += fr[(size_t)t * STOI_N + n];
            } else {
                if (t < T) a += fr[(size_t)t * STOI_N + n];
                if (t + 1 < T) a += fr[(size_t)(t + 1) * STOI_N + n - STOI_HOP];
            }
            g = fmaf(win[n], a, g);
        }
    }
    grad[(long long)b * grad_stride + s] = g;
}

extern "C" long long eab_stoi_bwd_workspace_bytes(int B, int cap) {
    const int FC = eab_stoi_frame_capacity(cap);
    if (B <= 0 || B > 65535 || FC < 0) return -1;
    return (long long)stoi_bwd_layout(B, FC).total;
}

extern "C" int eab_stoi_bwd_f32(const float* est, long long est_stride, int est_cap, int clean_cap, const int32_t* lens, int B,
                                const void* value_work, long long value_work_bytes, double factor_stoi, double factor_estoi,
                                const float* grad_out, int grad_out_stride, double scale, void* work, long long work_bytes, float* grad,
                                long long grad_stride, eab_stream_t stream) {
    EAB_CHECK_ARG(est && lens && value_work && grad_out && work && grad);
    EAB_CHECK_ARG(B >= 1 && B <= 65535 && est_cap > 0 && est_cap <= EAB_ROWS_MAX_LEN && clean_cap > 0 && clean_cap <= EAB_ROWS_MAX_LEN);
    EAB_CHECK_ARG(B == 1 || (est_stride >= est_cap && grad_stride >= est_cap));
    EAB_CHECK_ARG(grad_out_stride >= 0 && factor_stoi >= 0.0 && factor_estoi >= 0.0 && factor_stoi + factor_estoi > 0.0);
    EAB_CHECK_ARG(factor_stoi + factor_estoi < INFINITY && scale == scale && scale > -INFINITY && scale < INFINITY);
    EAB_CHECK_ARG(((reinterpret_cast<uintptr_t>(value_work) | reinterpret_cast<uintptr_t>(work)) & 15u) == 0);
    const int FC = eab_stoi_frame_capacity(est_cap > clean_cap ? est_cap : clean_cap);
    const StoiWork w = stoi_layout(B, FC);
    const StoiBwdWork wb = stoi_bwd_layout(B, FC);
    EAB_CHECK_ARG(value_work_bytes >= (long long)w.total && work_bytes >= (long long)wb.total);
    const StoiRows rows = {{nullptr, est}, {0, est_stride}, {clean_cap, est_cap}};      // (the clean rows are not read again)
    const char* vb = static_cast<const char*>(value_work);
    const float* win = reinterpret_cast<const float*>(vb + w.win);
    const float2* tw = reinterpret_cast<const float2*>(vb + w.tw);
    const int32_t* kept = reinterpret_cast<const int32_t*>(vb + w.kept);
    const int32_t* K = reinterpret_cast<const int32_t*>(vb + w.K);
    const float* tob = reinterpret_cast<const float*>(vb + w.tob);
    char* base = static_cast<char*>(work);
    double* part = reinterpret_cast<double*>(base + wb.part);
    float* frames = reinterpret_cast<float*>(base + wb.frames);
    const int tiles = (FC + STOI_TILE - 1) / STOI_TILE;
    hipStream_t s = eab_stream(stream);
    hipLaunchKernelGGL(stoi_segments_bwd_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(STOI_THREADS), 0, s, FC, K, tob, grad_out,
                       grad_out_stride, factor_stoi * scale, factor_estoi * scale, part);
    hipLaunchKernelGGL(stoi_bands_bwd_kernel, dim3((unsigned)((FC + FFT_SIGS - 1) / FFT_SIGS), (unsigned)B), dim3(STOI_THREADS), 0, s,
                       rows, lens, FC, kept, K, win, tw, tob, part, frames);
    hipLaunchKernelGGL(stoi_gather_bwd_kernel, dim3((unsigned)((est_cap + STOI_THREADS - 1) / STOI_THREADS), (unsigned)B),
                       dim3(STOI_THREADS), 0, s, rows, lens, FC, kept, K, win, frames, grad, grad_stride);
    EAB_RETURN_LAUNCH_STATUS();
}
