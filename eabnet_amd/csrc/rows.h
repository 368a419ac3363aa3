// Padded rows of the scores and the wave losses (score.hip, wave_loss.hip, spec_loss.hip, stoi.hip, stoi_bwd.hip; optim.hip and
// stft.hip take single helpers): N signals, each a [B][stride] array of which the first cap floats of a row may be read and the
// first lens[b] of them are the utterance; the spans a row is cut into and their fixed-order reduction; the reflect index of a
// centred frame.  Plain C++ and f32x4 only: all but stft.hip also compile as host C++ against tests/hip_host_shim.
#pragma once
#include "common.h"

#define EAB_ROWS_MAX_LEN (1 << 30)
#define EAB_SPAN_THREADS 256
#define EAB_SPAN 4096                         /* samples (bins) per workgroup and partial row: 4 rounds of 256 lanes x 4 samples */

template <int N>
struct EabRows {
    const float* p[N];
    long long stride[N];          // floats between the rows of two utterances
    int cap[N];                   // floats of a row that may be read
};

// the checks every entry point on rows makes: 1 <= B <= 65535, every capacity in (0, 2^30], and rows of two utterances that do not
// overlap (B = 1 has no second row)
template <int N>
static inline bool eab_rows_ok(const EabRows<N>& rows, int B) {
    if (B < 1 || B > 65535) return false;
    for (int k = 0; k < N; ++k) {
        if (!rows.p[k] || rows.cap[k] <= 0 || rows.cap[k] > EAB_ROWS_MAX_LEN) return false;
        if (B > 1 && rows.stride[k] < rows.cap[k]) return false;
    }
    return true;
}

// spans of a row of n samples, and of the longest capacity of these rows: what an entry point asks of its `partial_spans`
static inline int eab_spans(int n) { return (n + EAB_SPAN - 1) / EAB_SPAN; }
template <int N>
static inline int eab_rows_spans(const EabRows<N>& rows) {
    int cap = rows.cap[0];
    for (int k = 1; k < N; ++k) cap = rows.cap[k] > cap ? rows.cap[k] : cap;
    return eab_spans(cap);
}

__device__ __forceinline__ int eab_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// samples of signal k of utterance b: lens is [B][N], the device content clamped into the row
template <int N>
__device__ __forceinline__ int eab_len(const int32_t* __restrict__ lens, const EabRows<N>& rows, int b, int k) {
    return eab_clamp(lens[N * b + k], rows.cap[k]);
}
__device__ __forceinline__ bool eab_aligned16(const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// four consecutive values of a row at index i (a multiple of four); zero at and past len.  A row that is 16-byte aligned loads its
// four as one dwordx4, any other row (and the quad that straddles len) one by one AT THE SAME indices: the same bits either way.
__device__ __forceinline__ void eab_load4(const float* __restrict__ row, bool aligned, int i, int len, float v[4]) {
    if (aligned && i + 4 <= len) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(row + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i + k < len ? row[i + k] : 0.0f;
    }
}

// first index of lane `tid`'s quad j of span `span`: inside a span a lane owns j * 1024 + 4 * tid + {0..3}, j = 0..3, in that order
__device__ __forceinline__ int eab_span_quad(int span, int j, int tid) {
    return span * EAB_SPAN + j * 4 * EAB_SPAN_THREADS + 4 * tid;
}

// acc[0..NQ) of all 256 lanes -> dst[0..NQ): shuffle tree in the wave, waves 0..3 in order
template <int NQ>
__device__ __forceinline__ void eab_span_reduce(double acc[NQ], double* __restrict__ dst) {
    __shared__ double red[EAB_SPAN_THREADS / 64][NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_down(acc[q], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int q = 0; q < NQ; ++q) red[wave][q] = acc[q];
    __syncthreads();
    if (threadIdx.x < NQ) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < EAB_SPAN_THREADS / 64; ++w) s += red[w][threadIdx.x];
        dst[threadIdx.x] = s;
    }
}

// reflect_pad(x, P)[i] for i in [0, n + 2P) as an index into the n samples; P < n: one reflection at most
__device__ __forceinline__ int eab_reflect(int i, int P, int n) {
    int j = i - P;
    if (j < 0) j = -j;
    if (j >= n) j = 2 * (n - 1) - j;
    return j;
}
