// Windowed-sinc sample-rate conversion of the rows of a padded batch, on the device (what enhance.py:35-37 and test.py:65-68
// do per file on the host before the first STFT; the microphone reordering of enhance.py:41-42 rides along as a row map).
//
// For rates orig -> new, o = orig/gcd, n = new/gcd, output sample i = q*n + p (phase p in [0, n)) of a row x is
//     y[i] = sum_{k < K} tab[p][k] * x[q*o + first[p] + k]            (x = 0 outside [0, valid end))
// with the polyphase bank (tab, first) of eabnet_amd/resample.py filter_bank: first[p] is nondecreasing in p and
// first[n-1] - first[0] <= o.  The sum runs in ascending k in fp32, every step one explicit fmaf (the build has
// -ffp-contract=off), and the zero-padded taps of a short phase are multiplied like the others: ONE order per output sample,
// so its bits do not depend on the batch, on the tile it falls in or on where a stream was cut.
//
// Positions: in_origin / out_origin are the absolute indices of x[., 0] and y[., 0] (64-bit: a day at 48 kHz passes 2^32).  A
// workgroup owns R*256 consecutive outputs of one row; it takes the 64-bit quotient and phase of its first output once, and
// everything inside the tile is a 32-bit offset from there.
//
// Memory shape: the input span of the tile ((R*256/n + 2)*o + K floats at most) is staged into LDS with 16-byte loads from the
// first 16-byte boundary at or below its start -- whatever the row stride, the origin and the length do to the alignment -- and
// one by one, guarded, where a quad straddles the row's begin or valid end; samples outside the valid range are never read.
// The bank lives in LDS with an odd row pitch (lanes of consecutive phases hit different banks); for n == 1 its one row is read
// through uniform (scalar) loads instead.  Lane t owns outputs t, t+256, ... of the tile (coalesced 4-byte stores, R outputs in
// flight per k).  LDS read stride between lanes is o/n floats: conflict-free for odd o; for n == 1 and even o (32k, 96k -> 16k)
// the staged span is skewed by one float per 32 (index a -> a + a/32), which spreads a stride of 2, 4 or 8 over all 32 banks.
// Bound: LDS read issue (one or two ds_read_b32 per tap and lane), not HBM: DESIGN.md 4.15.
#include "common.h"

#define RS_THREADS 256
#define RS_MAX_BANK 16384                     /* floats of tab: 64 KB */
#define RS_MAX_SPAN 12288                     /* floats of a tile's staged input span */
#define RS_MAX_COLS (1 << 30)

struct ResampleArgs {
    const float* x; long long x_row_stride; int x_cols; const int32_t* row_map; const int32_t* in_lens; int rows_per_utt;
    float* y; long long y_row_stride; int n_out;
    const float* tab; const int32_t* first; int o, n, K;
    long long in_origin, out_origin, valid_hi;
    int span_cap;                             // floats of the staged span the launch reserved
};

template <bool SKEW>
__device__ __forceinline__ int rs_pos(int a) { return SKEW ? a + (a >> 5) : a; }

// R outputs per lane; ONE: n == 1 (one phase, the taps through scalar loads); SKEW: skewed span (n == 1, even o)
template <int R, bool ONE, bool SKEW>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int tid = threadIdx.x, row = blockIdx.y, o = a.o, n = ONE ? 1 : a.n, K = a.K;
    const int Kp = K | 1;                                           // odd pitch of the bank's rows in LDS
    float* tabs = rs_lds;                                           // [n][Kp]              (ONE: absent)
    int* firsts = reinterpret_cast<int*>(rs_lds + (ONE ? 0 : n * Kp));   // [n]             (ONE: absent)
    float* xs = rs_lds + (ONE ? 0 : (n * Kp + n + 3) / 4 * 4);      // the tile's input span

    const int j0 = blockIdx.x * (R * RS_THREADS);                   // first output of the tile, relative to y[., 0]
    const int j1 = min(j0 + R * RS_THREADS, a.n_out);
    const long long irow = a.row_map ? a.row_map[row] : row;
    const float* __restrict__ xr = a.x + irow * a.x_row_stride;
    float* __restrict__ yr = a.y + (long long)row * a.y_row_stride;

    // valid input samples [0, hi) relative to x[., 0]; outputs [0, out_hi) relative to y[., 0] are computed, the rest is zero
    long long hi64 = a.valid_hi < 0 ? (long long)a.x_cols : a.valid_hi - a.in_origin;
    int out_hi = a.n_out;
    if (a.in_lens) {
        const int len = a.in_lens[row / a.rows_per_utt];
        hi64 = min(hi64, (long long)len);
    }
    const int hi = (int)max(0LL, min(hi64, (long long)a.x_cols));
    if (a.in_lens) {
        const long long hi_abs = a.in_origin + hi;
        const long long oh = (hi_abs * n + o - 1) / o - a.out_origin;
        out_hi = (int)max(0LL, min(oh, (long long)a.n_out));
    }
    const int jend = min(j1, out_hi);                               // outputs [j0, jend) are sums, [jend, j1) zeros
    if (jend <= j0) {                                               // (workgroup-uniform)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = j0 + tid + r * RS_THREADS;
            if (j < j1) yr[j] = 0.0f;
        }
        return;
    }

    // the tile's 64-bit position, once
    const long long i0 = a.out_origin + j0;
    const long long q0 = i0 / n;
    const int p0 = (int)(i0 - q0 * n);
    long long base64 = q0 * o - a.in_origin;                        // input index of (q0, m = 0) relative to x[., 0]
    base64 = max(-(long long)RS_MAX_COLS, min(base64, (long long)RS_MAX_COLS));   // (farther out: all zeros anyway)
    const int base = (int)base64;
    const int s0 = base + a.first[p0];                              // first input sample the tile reads
    const int mis = (int)((reinterpret_cast<uintptr_t>(xr) >> 2) & 3u);
    const int s0a = s0 - ((s0 + mis) & 3);                          // ... moved down to a 16-byte boundary of the row
    const int pl = p0 + (jend - 1 - j0), ql = pl / n;
    const int need = min(base + ql * o + a.first[pl - ql * n] + K - s0a, a.span_cap);

    for (int c = 4 * tid; c < need; c += 4 * RS_THREADS) {
        const int e = s0a + c;
        float v[4];
        if (e >= 0 && e + 4 <= hi) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(xr + e);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (e + k >= 0 && e + k < hi) ? xr[e + k] : 0.0f;
        }
        const int d = rs_pos<SKEW>(c);                              // (a quad never crosses a multiple of 32)
#pragma unroll
        for (int k = 0; k < 4; ++k) xs[d + k] = v[k];
    }
    if (!ONE) {
        for (int p = tid; p < n; p += RS_THREADS) firsts[p] = a.first[p];
        for (int idx = tid; idx < n * K; idx += RS_THREADS) {
            const int p = idx / K;
            tabs[p * Kp + (idx - p * K)] = a.tab[idx];
        }
    }
    __syncthreads();

    float acc[R];
    int xb[R], tb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int pj = p0 + tid + r * RS_THREADS;
        const int q = ONE ? pj : pj / n, p = ONE ? 0 : pj - q * n;
        const int b = base + q * o + (ONE ? a.first[0] : firsts[p]) - s0a;
        xb[r] = max(0, min(b, a.span_cap - K));                     // (a lane past jend may point anywhere: keep it inside)
        tb[r] = p * Kp;
        acc[r] = 0.0f;
    }
    const float* __restrict__ tab1 = a.tab;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float t = ONE ? tab1[k] : tabs[tb[r] + k];
            acc[r] = fmaf(t, xs[rs_pos<SKEW>(xb[r] + k)], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = j0 + tid + r * RS_THREADS;
        if (j < jend) yr[j] = acc[r];
        else if (j < j1) yr[j] = 0.0f;
    }
}

// floats of LDS span a tile of `tile` outputs may need: (tile/n + 1) steps of o between its first and last quotient, the
// spread of first[] (<= o), K taps, and the slack of the 16-byte alignment at both ends
static inline long long rs_span(int tile, int o, int n, int K) { return ((long long)tile / n + 2) * o + K + 8; }

template <int R, bool ONE, bool SKEW>
static int rs_launch(ResampleArgs& a, int rows, eab_stream_t stream) {
    a.span_cap = (int)rs_span(R * RS_THREADS, a.o, a.n, a.K);
    const int span_floats = (SKEW ? a.span_cap + (a.span_cap >> 5) + 1 : a.span_cap) + 4;   // (+4: the last staged quad)
    const int Kp = a.K | 1;
    const size_t lds = sizeof(float) * ((ONE ? 0 : (a.n * Kp + a.n + 3) / 4 * 4) + (size_t)span_floats);
    const void* fn = reinterpret_cast<const void*>(&resample_kernel<R, ONE, SKEW>);
    if (lds > 64 * 1024) {
        EAB_CHECK_ARG(lds <= 160 * 1024);
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return eab_hip_status(e);
    }
    const unsigned tiles = (unsigned)((a.n_out + R * RS_THREADS - 1) / (R * RS_THREADS));
    hipLaunchKernelGGL((resample_kernel<R, ONE, SKEW>), dim3(tiles, (unsigned)rows), dim3(RS_THREADS), lds, eab_stream(stream), a);
    EAB_RETURN_LAUNCH_STATUS();
}

extern "C" int eab_resample_f32(const float* x, long long x_row_stride, int x_cols, const int32_t* row_map, const int32_t* in_lens,
                                int rows, int rows_per_utt, float* y, long long y_row_stride, int n_out, const float* tab,
                                const int32_t* first, int o, int n, int K, long long in_origin, long long out_origin,
                                long long valid_hi, eab_stream_t stream) {
    EAB_CHECK_ARG(x && y && tab && first);
    EAB_CHECK_ARG(o >= 1 && n >= 1 && K >= 1 && (long long)K * n <= RS_MAX_BANK);
    EAB_CHECK_ARG(rows >= 0 && rows <= 65535 && rows_per_utt >= 1 && x_cols >= 0 && x_cols <= RS_MAX_COLS && n_out >= 0);
    EAB_CHECK_ARG(in_origin >= 0 && out_origin >= 0 && in_origin <= (1LL << 46) && out_origin <= (1LL << 46));
    EAB_CHECK_ARG(valid_hi < 0 || valid_hi <= (1LL << 47));
    EAB_CHECK_ARG(y_row_stride >= n_out || rows <= 1);
    const bool four = rs_span(4 * RS_THREADS, o, n, K) <= RS_MAX_SPAN;
    EAB_CHECK_ARG(four || rs_span(RS_THREADS, o, n, K) <= RS_MAX_SPAN);      // a decimation too steep for one tile's LDS
    if (rows == 0 || n_out == 0) return EAB_OK;
    ResampleArgs a{x, x_row_stride, x_cols, row_map, in_lens, rows_per_utt, y, y_row_stride, n_out, tab, first, o, n, K,
                   in_origin, out_origin, valid_hi, 0};
    if (n == 1) {
        if (o % 2 == 0) return four ? rs_launch<4, true, true>(a, rows, stream) : rs_launch<1, true, true>(a, rows, stream);
        return four ? rs_launch<4, true, false>(a, rows, stream) : rs_launch<1, true, false>(a, rows, stream);
    }
    return four ? rs_launch<4, false, false>(a, rows, stream) : rs_launch<1, false, false>(a, rows, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The adjoint of the whole-signal resampler (both origins 0, no row map): input sample j of a row collects
//     gx[j] = sum tab[p][k] * gy[q*n + p]       over the (q, p, k) with q*o + first[p] + k == j
// as a gather, one thread per input sample, in ascending output index q*n + p and one fmaf per term: ONE order per sample, so its
// bits do not depend on the batch.  For a quotient q the phases that reach j are those with j - q*o - K < first[p] <= j - q*o: one
// run of p, because first[] is nondecreasing, found by two binary searches.  Outputs at and past ceil(n*len/o) carry no gradient
// (the forward wrote zeros there) and gx is zero from len on.  The bank and gy are read through the caches: a sample takes about
// K*n/o terms (12 at 16 -> 10 kHz).
struct ResampleBwdArgs {
    const float* gy; long long gy_row_stride; int n_out; const int32_t* in_lens; int rows_per_utt;
    float* gx; long long gx_row_stride; int x_cols;
    const float* tab; const int32_t* first; int o, n, K;
};

__device__ __forceinline__ int rs_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// the first p in [0, n) with first[p] > v (n if none)
__device__ __forceinline__ int rs_first_above(const int32_t* __restrict__ first, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(RS_THREADS) void resample_bwd_kernel(const ResampleBwdArgs a) {
    const int j = blockIdx.x * RS_THREADS + threadIdx.x, row = blockIdx.y;
    if (j >= a.x_cols) return;
    const int o = a.o, n = a.n, K = a.K;
    int hi = a.x_cols, out_hi = a.n_out;
    if (a.in_lens) {
        hi = max(0, min(a.in_lens[row / a.rows_per_utt], a.x_cols));
        out_hi = (int)min((long long)a.n_out, ((long long)hi * n + o - 1) / o);
    }
    float acc = 0.0f;
    if (j < hi) {
        const float* __restrict__ gyr = a.gy + (long long)row * a.gy_row_stride;
        const int q_lo = max(0, rs_floor_div(j - a.first[n - 1] - K, o) + 1), q_hi = rs_floor_div(j - a.first[0], o);
        for (int q = q_lo; q <= q_hi; ++q) {
            const int r = j - q * o;                                    // first[p] + k == r with 0 <= k < K
            const int p_end = rs_first_above(a.first, n, r);
            for (int p = rs_first_above(a.first, n, r - K); p < p_end; ++p) {
                const long long i = (long long)q * n + p;
                if (i >= out_hi) break;
                acc = fmaf(a.tab[p * K + (r - a.first[p])], gyr[i], acc);
            }
        }
    }
    a.gx[(long long)row * a.gx_row_stride + j] = acc;
}

extern "C" int eab_resample_bwd_f32(const float* gy, long long gy_row_stride, int n_out, const int32_t* in_lens, int rows,
                                    int rows_per_utt, float* gx, long long gx_row_stride, int x_cols, const float* tab,
                                    const int32_t* first, int o, int n, int K, eab_stream_t stream) {
    EAB_CHECK_ARG(gy && gx && tab && first);
    EAB_CHECK_ARG(o >= 1 && n >= 1 && K >= 1 && (long long)K * n <= RS_MAX_BANK);
    EAB_CHECK_ARG(rows >= 0 && rows <= 65535 && rows_per_utt >= 1 && x_cols >= 0 && x_cols <= RS_MAX_COLS && n_out >= 0);
    EAB_CHECK_ARG(rows <= 1 || (gy_row_stride >= n_out && gx_row_stride >= x_cols));
    if (rows == 0 || x_cols == 0) return EAB_OK;
    const ResampleBwdArgs a{gy, gy_row_stride, n_out, in_lens, rows_per_utt, gx, gx_row_stride, x_cols, tab, first, o, n, K};
    hipLaunchKernelGGL(resample_bwd_kernel, dim3((unsigned)((x_cols + RS_THREADS - 1) / RS_THREADS), (unsigned)rows), dim3(RS_THREADS),
                       0, eab_stream(stream), a);
    EAB_RETURN_LAUNCH_STATUS();
}
