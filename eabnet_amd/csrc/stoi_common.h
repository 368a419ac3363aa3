// What the kernels of the value (stoi.hip) and of the gradient (stoi_bwd.hip) share: the constants of DESIGN §4.16, the rows, the
// layout of the value call's workspace (which the gradient reads) and the clamped lengths.
#pragma once
#include "rows.h"

#define STOI_THREADS 256
#define STOI_N 256                            /* samples of a frame */
#define STOI_HOP 128
#define STOI_BANDS 15
#define STOI_SEG 30                           /* frames of a segment */
#define STOI_BIN_LO 7                         /* bins [7, 219) carry the 15 bands */
#define STOI_BIN_HI 219
#define STOI_EFRAMES 16                       /* frames per workgroup of kernel 1 */
#define STOI_TILE 16                          /* segments per workgroup of kernel 4 */
#define STOI_TILE_FRAMES (STOI_TILE + STOI_SEG - 1)
#define STOI_EPS 2.220446049250313e-16        /* 2^-52 */

// band i sums the bins [stoi_edge[i], stoi_edge[i + 1])
__device__ const int stoi_edge[STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

typedef EabRows<2> StoiRows;        // clean, processed

struct StoiWork {                 // byte offsets into the workspace
    size_t win, tw, energy, kept, K, tob, partial, total;
};

static inline int stoi_frames_host(long long L) { return L > STOI_N ? (int)((L - STOI_N + STOI_HOP - 1) / STOI_HOP) : 0; }
__device__ __forceinline__ int stoi_frames(int L) { return L > STOI_N ? (L - STOI_N + STOI_HOP - 1) / STOI_HOP : 0; }

static StoiWork stoi_layout(int B, int FC) {
    const size_t tiles = (size_t)(FC + STOI_TILE - 1) / STOI_TILE;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    StoiWork w;
    w.win = 0;
    w.tw = up(w.win + STOI_N * sizeof(float));
    w.energy = up(w.tw + 2 * STOI_N * sizeof(float2));
    w.kept = up(w.energy + (size_t)B * FC * sizeof(double));
    w.K = up(w.kept + (size_t)B * FC * sizeof(int32_t));
    w.tob = up(w.K + (size_t)B * sizeof(int32_t));
    w.partial = up(w.tob + (size_t)B * 2 * STOI_BANDS * FC * sizeof(float));
    w.total = up(w.partial + (size_t)B * tiles * 2 * sizeof(double));
    return w;
}

// lens [B][2] = samples of (processed, clean): the order of the Python call's (est, clean)
__device__ __forceinline__ void stoi_lens(const int32_t* __restrict__ lens, const StoiRows& rows, int b, int& ls, int& le) {
    le = eab_clamp(lens[2 * b], rows.cap[1]);
    ls = eab_clamp(lens[2 * b + 1], rows.cap[0]);
}
