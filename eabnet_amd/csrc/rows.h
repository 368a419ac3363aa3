// Padded rows of the file tools (score.hip, stoi.hip): N signals, each a [B][stride] array of which the first cap floats of a row
// may be read and the first lens[b] of them are the utterance.  Plain C++ and f32x4 only: both files also compile as host C++
// against tests/hip_host_shim.
#pragma once
#include "common.h"

#define EAB_ROWS_MAX_LEN (1 << 30)

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

__device__ __forceinline__ int eab_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
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
