// Intelligibility scores per utterance of a padded batch, on the device: STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) of
// cal_single_metrics (reference test.py:126-153), at 10 kHz.  The definition is the contract; equality with a host
// STOI library is not verified.
//
// x = clean, y = processed, both zero from their own length up to the longer one (never read there).  With w the 256 inner points of
// a 258-point Hann window, frames of 256 at hop 128 while start + 256 < L:
//   1  stoi_energy_kernel    E[j] = sum_n (w[n] x[128 j + n])^2, fp64; one wave per frame, lane l owns samples 4l..4l+3 in that
//                            order, lanes by a fixed shuffle tree.  Workgroup (0, 0) also writes the fp32 window and the 512-point
//                            twiddle table (both rounded from fp64) into the workspace for kernel 3.
//   2  stoi_mask_kernel      per utterance: e_j = 20 log10(sqrt E[j] + eps), frame j kept iff max e - 40 - e_j < 0 (fp64, literal
//                            form), exclusive scan by ballots -> kept[t] (source frame of compacted frame t) and K.
//   3  stoi_bands_kernel     8 compacted frames of one signal per workgroup.  Frame t of the overlap-added signal is built in LDS
//                            straight from the source (three source frames, each 256 contiguous samples, four per lane),
//                            windowed again, transformed as a 256-point complex FFT of the even/odd-packed 512-point real frame
//                            (fft_lds.h passes 4 . 8 . 8), untangled for bins 7..218 only, and the 15 third-octave band sums
//                            (fp64, ascending bin) are stored as sqrt in fp32: tob[b][signal][band][t], t < T = K - 1.
//   4  stoi_segments_kernel  16 segments of 30 frames per workgroup, thread (segment, band): the fp64 statistics of both scores
//                            from an LDS tile of 45 frames; ESTOI's column pass by thread (segment, two columns).  One partial
//                            pair per tile: bands / columns, then the tile's segments, added in index order.
//   5  stoi_final_kernel     per utterance: the tiles in index order, / (15 S) and / (30 S); 1e-5 for T < 30.
// Nothing synchronises with the host: K is device data, the grids are sized from the frame capacity and workgroups beyond an
// utterance's frames, K or T leave before their first barrier.  Determinism: every sum has one order that depends on the
// utterance alone (frame, tile and segment indices count from the utterance's start; a row that is 16-byte aligned loads four
// samples at once, any other one by one AT THE SAME indices); no atomics.  An utterance has the same bits alone, in any batch
// and in a second call.
// Bound: launch latency; kernel 3 reads every kept sample twice (L2) and does ~25 kFLOP per frame.
#include "stoi_common.h"
#include "fft_lds.h"

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(STOI_THREADS) void stoi_energy_kernel(const StoiRows rows, const int32_t* __restrict__ lens, int FC,
                                                                   double* __restrict__ energy, float* __restrict__ win_out,
                                                                   float2* __restrict__ tw_out) {
    __shared__ double w[STOI_N];
    const int tid = threadIdx.x, b = blockIdx.y;
    const double wv = 0.5 - 0.5 * cospi(2.0 * (double)(tid + 1) / (double)(STOI_N + 1));
    if (blockIdx.x == 0 && b == 0) {                                    // the tables of kernel 3
        win_out[tid] = (float)wv;
        for (int j = tid; j < 2 * STOI_N; j += STOI_THREADS) {
            const double a = (double)j / (double)STOI_N;                // exp(-2 pi i j / 512)
            tw_out[j] = make_float2((float)cospi(a), (float)(-sinpi(a)));
        }
    }
    int ls, le;
    stoi_lens(lens, rows, b, ls, le);
    const int NF = stoi_frames(max(ls, le));
    const int j0 = blockIdx.x * STOI_EFRAMES;
    if (j0 >= NF) return;                                               // (workgroup-uniform, before the barrier)
    w[tid] = wv;
    __syncthreads();
    const float* x = rows.p[0] + (long long)b * rows.stride[0];
    const bool al = eab_aligned16(x);
    const int lane = tid & 63, wave = tid >> 6;
    for (int f = wave; f < STOI_EFRAMES; f += STOI_THREADS / 64) {
        const int j = j0 + f;
        if (j >= NF) break;                                             // (wave-uniform)
        float v[4];
        eab_load4(x, al, STOI_HOP * j + 4 * lane, ls, v);
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double p = w[4 * lane + k] * (double)v[k];
            acc += p * p;
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (lane == 0) energy[(size_t)b * FC + j] = acc;
    }
}

__device__ __forceinline__ double stoi_db(double energy) { return 20.0 * log10(sqrt(energy) + STOI_EPS); }

__global__ __launch_bounds__(STOI_THREADS) void stoi_mask_kernel(const StoiRows rows, const int32_t* __restrict__ lens, int FC,
                                                                 const double* __restrict__ energy, int32_t* __restrict__ kept,
                                                                 int32_t* __restrict__ K) {
    __shared__ double wmax[STOI_THREADS / 64];
    __shared__ int wcnt[STOI_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    int ls, le;
    stoi_lens(lens, rows, b, ls, le);
    const int NF = stoi_frames(max(ls, le));
    const double* en = energy + (size_t)b * FC;
    int32_t* kp = kept + (size_t)b * FC;
    double m = -INFINITY;
    for (int j = tid; j < NF; j += STOI_THREADS) m = fmax(m, stoi_db(en[j]));
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    m = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
    int base = 0;
    for (int c0 = 0; c0 < NF; c0 += STOI_THREADS) {                     // (NF is workgroup-uniform)
        const int j = c0 + tid;
        bool keep = false;
        if (j < NF) keep = m - 40.0 - stoi_db(en[j]) < 0.0;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int off = base, total = 0;
        for (int q = 0; q < STOI_THREADS / 64; ++q) {
            if (q < wave) off += wcnt[q];
            total += wcnt[q];
        }
        if (keep) kp[off + __popcll(bal & ((1ull << lane) - 1ull))] = j;
        base += total;
        __syncthreads();
    }
    if (tid == 0) K[b] = base;
}

// ---------------------------------------------------------------------------------------------------------------------------------
#define STOI_P_STRIDE (STOI_N + 1)            /* floats between the power rows of two frames: frames on different banks */

__global__ __launch_bounds__(STOI_THREADS) void stoi_bands_kernel(const StoiRows rows, const int32_t* __restrict__ lens, int FC,
                                                                  const int32_t* __restrict__ kept, const int32_t* __restrict__ K,
                                                                  const float* __restrict__ win_tab, const float2* __restrict__ tw_tab,
                                                                  float* __restrict__ tob) {
    __shared__ __attribute__((aligned(16))) float2 tw[2 * STOI_N];       // exp(-2 pi i j / 512)
    __shared__ __attribute__((aligned(16))) float2 buf0[FFT_SIGS * STOI_N + FFT_SIGS];   // (+ the padding of the power rows)
    __shared__ __attribute__((aligned(16))) float2 buf1[FFT_SIGS * STOI_N];
    __shared__ __attribute__((aligned(16))) float win[STOI_N];
    __shared__ int src[FFT_SIGS + 2];                                   // kept[t0 - 1 .. t0 + 8], -1 outside [0, K)
    const int tid = threadIdx.x, sig = blockIdx.y, b = blockIdx.z;
    const int Kb = K[b], T = Kb - 1, t0 = blockIdx.x * FFT_SIGS;
    if (t0 >= T) return;                                                // (workgroup-uniform, before any barrier)
    int ls, le;
    stoi_lens(lens, rows, b, ls, le);
    const int len = sig ? le : ls;
    const float* x = rows.p[sig] + (long long)b * rows.stride[sig];
    const bool al = eab_aligned16(x);
    tw[tid] = tw_tab[tid];
    tw[tid + STOI_N] = tw_tab[tid + STOI_N];
    win[tid] = win_tab[tid];
    if (tid < FFT_SIGS + 2) {
        const int t = t0 - 1 + tid;
        src[tid] = (t >= 0 && t < Kb) ? kept[(size_t)b * FC + t] : -1;
    }
    __syncthreads();
    // compacted frame t = 256 samples of the overlap-added signal at 128 t: its own source frame plus the second half of the one
    // before (n < 128) or the first half of the one after (n >= 128), each windowed once; then the window of the second framing.
    // One wave per frame, lane l owns samples 4l..4l+3: every wave-instruction reads one contiguous piece of one source frame.
    const int lane = tid & 63, wave = tid >> 6;
    for (int f = wave; f < FFT_SIGS; f += STOI_THREADS / 64) {
        const int n = 4 * lane;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t0 + f < T) {                                               // (wave-uniform)
            float own[4], nb[4] = {0.f, 0.f, 0.f, 0.f};
            eab_load4(x, al, STOI_HOP * src[f + 1] + n, len, own);
            const int other = n < STOI_HOP ? src[f] : src[f + 2], on = n < STOI_HOP ? n + STOI_HOP : n - STOI_HOP;
            if (other >= 0) eab_load4(x, al, STOI_HOP * other + on, len, nb);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (win[n + k] * own[k] + win[on + k] * nb[k]) * win[n + k];
        }
        float* z = reinterpret_cast<float*>(buf0) + f * 2 * STOI_N;     // float index 2 (n/2) + (n & 1) = n; the upper half is zero
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
    // X[k] = E[k] + W_512^k O[k],  E = (Z[k] + conj Z[256-k]) / 2,  O = (Z[k] - conj Z[256-k]) / 2i, for the bins of the bands
    float* P = reinterpret_cast<float*>(buf0);
    for (int e = tid; e < FFT_SIGS * (STOI_BIN_HI - STOI_BIN_LO); e += STOI_THREADS) {
        const int f = e / (STOI_BIN_HI - STOI_BIN_LO), k = STOI_BIN_LO + e - f * (STOI_BIN_HI - STOI_BIN_LO);
        const float2 z = buf1[f * STOI_N + k], zc = buf1[f * STOI_N + STOI_N - k];
        const float2 E = make_float2(0.5f * (z.x + zc.x), 0.5f * (z.y - zc.y));
        const float2 O = make_float2(0.5f * (z.y + zc.y), 0.5f * (zc.x - z.x));
        const float2 wo = cmul(tw[k], O);
        const float re = E.x + wo.x, im = E.y + wo.y;
        P[f * STOI_P_STRIDE + k] = re * re + im * im;
    }
    __syncthreads();
    if (tid < FFT_SIGS * STOI_BANDS) {
        const int f = tid & (FFT_SIGS - 1), band = tid >> 3;            // eight consecutive t per band: contiguous stores
        static_assert(FFT_SIGS == 8, "band = tid >> 3");
        if (t0 + f < T) {
            double s = 0.0;
            for (int k = stoi_edge[band]; k < stoi_edge[band + 1]; ++k) s += (double)P[f * STOI_P_STRIDE + k];
            tob[(((size_t)b * 2 + sig) * STOI_BANDS + band) * FC + t0 + f] = (float)sqrt(s);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
#define STOI_TILE_STRIDE (STOI_TILE_FRAMES + 4)

__global__ __launch_bounds__(STOI_THREADS) void stoi_segments_kernel(int FC, int tiles, const int32_t* __restrict__ K,
                                                                     const float* __restrict__ tob, double* __restrict__ partial) {
    __shared__ float tile[2][STOI_BANDS][STOI_TILE_STRIDE];             // frames s0 .. s0 + 44 of both signals
    __shared__ double rowst[STOI_TILE][STOI_BANDS][4];                  // ESTOI rows: mean and 1 / (norm + eps) of x and of y
    __shared__ double dband[STOI_TILE][STOI_BANDS];
    __shared__ double dcol[STOI_TILE][STOI_SEG];
    __shared__ double dseg[STOI_TILE][2];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int T = K[b] - 1, S = T - (STOI_SEG - 1), s0 = blockIdx.x * STOI_TILE;
    if (S <= 0 || s0 >= S) return;                                      // (workgroup-uniform, before any barrier)
    for (int e = tid; e < 2 * STOI_BANDS * STOI_TILE_FRAMES; e += STOI_THREADS) {
        const int r = e / STOI_TILE_FRAMES, fr = e - r * STOI_TILE_FRAMES;           // r = signal * 15 + band
        const int t = s0 + fr;
        (&tile[0][0][0])[r * STOI_TILE_STRIDE + fr] = t < T ? tob[((size_t)b * 2 * STOI_BANDS + r) * FC + t] : 0.0f;
    }
    __syncthreads();
    const int sl = tid >> 4, i = tid & 15;
    const bool active = i < STOI_BANDS && s0 + sl < S;
    const double inv_n = 1.0 / (double)STOI_SEG;
    if (active) {
        const float* xr = &tile[0][i][sl];
        const float* yr = &tile[1][i][sl];
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0;
        for (int t = 0; t < STOI_SEG; ++t) {
            const double xv = (double)xr[t], yv = (double)yr[t];
            sx += xv; sy += yv; sxx += xv * xv; syy += yv * yv;
        }
        const double alpha = sqrt(sxx) / (sqrt(syy) + STOI_EPS);
        const double clip = 1.0 + 5.623413251903491;                    // 1 + 10^(15/20)
        const double mx = sx * inv_n, my = sy * inv_n;
        double sp = 0.0, cxx = 0.0, cyy = 0.0;
        for (int t = 0; t < STOI_SEG; ++t) {
            const double xv = (double)xr[t], yv = (double)yr[t];
            sp += fmin(alpha * yv, clip * xv);
            cxx += (xv - mx) * (xv - mx);
            cyy += (yv - my) * (yv - my);
        }
        const double mp = sp * inv_n;
        double cpp = 0.0;
        for (int t = 0; t < STOI_SEG; ++t) {
            const double pv = fmin(alpha * (double)yr[t], clip * (double)xr[t]) - mp;
            cpp += pv * pv;
        }
        const double rx = 1.0 / (sqrt(cxx) + STOI_EPS), ry = 1.0 / (sqrt(cyy) + STOI_EPS), rp = 1.0 / (sqrt(cpp) + STOI_EPS);
        double d = 0.0;
        for (int t = 0; t < STOI_SEG; ++t) {
            const double xv = (double)xr[t], pv = fmin(alpha * (double)yr[t], clip * xv);
            d += ((xv - mx) * rx) * ((pv - mp) * rp);
        }
        dband[sl][i] = d;
        rowst[sl][i][0] = mx; rowst[sl][i][1] = rx; rowst[sl][i][2] = my; rowst[sl][i][3] = ry;
    }
    __syncthreads();
    if (active) {                                                       // ESTOI: the row-normalised columns i and i + 15
        const double inv_j = 1.0 / (double)STOI_BANDS;
        for (int c = i; c < STOI_SEG; c += STOI_BANDS) {
            double sx = 0.0, sy = 0.0;
            for (int r = 0; r < STOI_BANDS; ++r) {
                sx += ((double)tile[0][r][sl + c] - rowst[sl][r][0]) * rowst[sl][r][1];
                sy += ((double)tile[1][r][sl + c] - rowst[sl][r][2]) * rowst[sl][r][3];
            }
            const double mx = sx * inv_j, my = sy * inv_j;
            double cxx = 0.0, cyy = 0.0;
            for (int r = 0; r < STOI_BANDS; ++r) {
                const double xv = ((double)tile[0][r][sl + c] - rowst[sl][r][0]) * rowst[sl][r][1] - mx;
                const double yv = ((double)tile[1][r][sl + c] - rowst[sl][r][2]) * rowst[sl][r][3] - my;
                cxx += xv * xv;
                cyy += yv * yv;
            }
            const double rx = 1.0 / (sqrt(cxx) + STOI_EPS), ry = 1.0 / (sqrt(cyy) + STOI_EPS);
            double d = 0.0;
            for (int r = 0; r < STOI_BANDS; ++r) {
                const double xv = ((double)tile[0][r][sl + c] - rowst[sl][r][0]) * rowst[sl][r][1] - mx;
                const double yv = ((double)tile[1][r][sl + c] - rowst[sl][r][2]) * rowst[sl][r][3] - my;
                d += (xv * rx) * (yv * ry);
            }
            dcol[sl][c] = d;
        }
    }
    __syncthreads();
    if (active && i == 0) {
        double a = 0.0, e = 0.0;
        for (int r = 0; r < STOI_BANDS; ++r) a += dband[sl][r];
        for (int c = 0; c < STOI_SEG; ++c) e += dcol[sl][c];
        dseg[sl][0] = a;
        dseg[sl][1] = e;
    }
    __syncthreads();
    if (tid == 0) {
        const int n = min(STOI_TILE, S - s0);
        double a = 0.0, e = 0.0;
        for (int q = 0; q < n; ++q) { a += dseg[q][0]; e += dseg[q][1]; }
        double* o = partial + ((size_t)b * tiles + blockIdx.x) * 2;
        o[0] = a;
        o[1] = e;
    }
}

__global__ void stoi_final_kernel(int B, int tiles, const int32_t* __restrict__ K, const double* __restrict__ partial,
                                  double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int T = K[b] - 1, S = T - (STOI_SEG - 1);
    double a = 1e-5, e = 1e-5;                                          // fewer than 30 frames: the sentinel
    if (S > 0) {
        const int used = (S + STOI_TILE - 1) / STOI_TILE;
        a = e = 0.0;
        for (int k = 0; k < used; ++k) {
            a += partial[((size_t)b * tiles + k) * 2];
            e += partial[((size_t)b * tiles + k) * 2 + 1];
        }
        a /= (double)STOI_BANDS * (double)S;
        e /= (double)STOI_SEG * (double)S;
    }
    out[2 * b] = a;
    out[2 * b + 1] = e;
}

extern "C" int eab_stoi_frame_capacity(int cap) {
    if (cap <= 0 || cap > EAB_ROWS_MAX_LEN) return -1;
    const int f = stoi_frames_host(cap);
    return f > 0 ? f : 1;
}

extern "C" long long eab_stoi_workspace_bytes(int B, int cap) {
    const int FC = eab_stoi_frame_capacity(cap);
    if (B <= 0 || B > 65535 || FC < 0) return -1;
    return (long long)stoi_layout(B, FC).total;
}

extern "C" int eab_stoi_f32(const float* est, long long est_stride, int est_cap, const float* clean, long long clean_stride,
                            int clean_cap, const int32_t* lens, int B, void* work, long long work_bytes, double* out,
                            int32_t* tap_K, int32_t* tap_kept, float* tap_tob, eab_stream_t stream) {
    const StoiRows rows = {{clean, est}, {clean_stride, est_stride}, {clean_cap, est_cap}};
    EAB_CHECK_ARG(lens && work && out && eab_rows_ok(rows, B));
    EAB_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 15u) == 0);
    const int FC = eab_stoi_frame_capacity(est_cap > clean_cap ? est_cap : clean_cap);
    const StoiWork w = stoi_layout(B, FC);
    EAB_CHECK_ARG(work_bytes >= (long long)w.total);
    const int tiles = (FC + STOI_TILE - 1) / STOI_TILE;
    char* base = static_cast<char*>(work);
    float* win = reinterpret_cast<float*>(base + w.win);
    float2* tw = reinterpret_cast<float2*>(base + w.tw);
    double* energy = reinterpret_cast<double*>(base + w.energy);
    int32_t* kept = tap_kept ? tap_kept : reinterpret_cast<int32_t*>(base + w.kept);
    int32_t* K = tap_K ? tap_K : reinterpret_cast<int32_t*>(base + w.K);
    float* tob = tap_tob ? tap_tob : reinterpret_cast<float*>(base + w.tob);
    double* partial = reinterpret_cast<double*>(base + w.partial);
    hipStream_t s = eab_stream(stream);
    hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)((FC + STOI_EFRAMES - 1) / STOI_EFRAMES), (unsigned)B), dim3(STOI_THREADS), 0,
                       s, rows, lens, FC, energy, win, tw);
    hipLaunchKernelGGL(stoi_mask_kernel, dim3((unsigned)B), dim3(STOI_THREADS), 0, s, rows, lens, FC, energy, kept, K);
    hipLaunchKernelGGL(stoi_bands_kernel, dim3((unsigned)((FC + FFT_SIGS - 1) / FFT_SIGS), 2u, (unsigned)B), dim3(STOI_THREADS), 0, s,
                       rows, lens, FC, kept, K, win, tw, tob);
    hipLaunchKernelGGL(stoi_segments_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(STOI_THREADS), 0, s, FC, tiles, K, tob, partial);
    hipLaunchKernelGGL(stoi_final_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, B, tiles, K, partial, out);
    EAB_RETURN_LAUNCH_STATUS();
}
