// Stand-alone driver of the host emulation of csrc/optim.hip: eab_grad_sumsq_f64 (twice, for the same-bits contract) and
// eab_adam_clip_f32 on arrays allocated at their exact size, 16-byte aligned, the gradients optionally one float past such a
// boundary, so that AddressSanitizer sees any access past a segment.
//   optim_emulation IN OUT GRAD_OFFSET_FLOATS
// IN:  int32 nseg, double [7] max_norm step_size beta1 beta2 bias2_sqrt eps weight_decay, int64 [nseg] n,
//      then per segment the fp32 arrays param, grad, exp_avg, exp_avg_sq
// OUT: int64 chunks, double [chunks] partial of run 1, double [chunks] of run 2, double norm,
//      then per segment the fp32 arrays param, exp_avg, exp_avg_sq
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eabnet_hip.h"

static float* exact(long long n, int off) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, (size_t)(n + off) * sizeof(float) + (n + off == 0 ? 16 : 0))) exit(2);
    return static_cast<float*>(p) + off;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int off = atoi(argv[3]);
    int nseg = 0;
    double h[7];
    if (fread(&nseg, 4, 1, f) != 1 || nseg < 1 || nseg > 64 || fread(h, 8, 7, f) != 7) return 2;
    std::vector<long long> n(nseg);
    if (fread(n.data(), 8, nseg, f) != (size_t)nseg) return 2;
    std::vector<eab_optim_segment> segs(nseg);
    long long total = 0;
    for (int s = 0; s < nseg; ++s) {
        float* a[4] = {exact(n[s], 0), exact(n[s], off), exact(n[s], 0), exact(n[s], 0)};
        for (int k = 0; k < 4; ++k)
            if (fread(a[k], 4, n[s], f) != (size_t)n[s]) return 2;
        segs[s] = eab_optim_segment{a[0], a[1], a[2], a[3], n[s]};
        total += n[s];
    }
    fclose(f);
    const long long chunks = (total + EAB_OPTIM_CHUNK - 1) / EAB_OPTIM_CHUNK;
    std::vector<double> p1(chunks), p2(chunks);
    double norm = -1.0;
    int rc = eab_grad_sumsq_f64(segs.data(), nseg, p1.data(), chunks, nullptr);
    if (!rc) rc = eab_grad_sumsq_f64(segs.data(), nseg, p2.data(), chunks, nullptr);
    if (!rc) rc = eab_adam_clip_f32(segs.data(), nseg, p1.data(), chunks, h[0], h[1], h[2], h[3], h[4], h[5], h[6], &norm, nullptr);
    if (rc) {
        printf("optim entry point returned %d\n", rc);
        return 1;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&chunks, 8, 1, o);
    fwrite(p1.data(), 8, chunks, o);
    fwrite(p2.data(), 8, chunks, o);
    fwrite(&norm, 8, 1, o);
    for (int s = 0; s < nseg; ++s) {
        fwrite(segs[s].param, 4, n[s], o);
        fwrite(segs[s].exp_avg, 4, n[s], o);
        fwrite(segs[s].exp_avg_sq, 4, n[s], o);
    }
    fclose(o);
    return 0;
}
