// Stand-alone driver of the host emulation of csrc/stoi_bwd.hip: eab_stoi_f32 (no taps), then eab_stoi_bwd_f32
// on the workspace it left, on rows allocated at their exact size and poisoned with NaN past every utterance's own length; the
// gradient rows are allocated at their exact size too and start as NaN, so that a sample the kernels skip shows.
//   stoi_bwd_emulation IN OUT UNALIGNED FACTOR_STOI FACTOR_ESTOI
// IN:  int32 B, B x (int32 est samples, int32 clean samples), float [B] grad_out, the est rows, the clean rows (fp32, own lengths)
// OUT: int32 est capacity, double [B][2] scores, float [B][capacity] gradient
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eabnet_hip.h"

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int B = 0;
    if (fread(&B, 4, 1, f) != 1 || B < 1) return 2;
    std::vector<int> lens(2 * B);
    if (fread(lens.data(), 4, 2 * B, f) != (size_t)(2 * B)) return 2;
    std::vector<float> gout(B);
    if (fread(gout.data(), 4, B, f) != (size_t)B) return 2;
    int ecap = 0, scap = 0;
    for (int b = 0; b < B; ++b) {
        ecap = std::max(ecap, lens[2 * b]);
        scap = std::max(scap, lens[2 * b + 1]);
    }
    const int odd = atoi(argv[3]);                                    // the rows start 4 bytes past a 16-byte boundary
    const double fs = atof(argv[4]), fe = atof(argv[5]);
    std::vector<float> est((size_t)B * ecap + odd, NAN), clean((size_t)B * scap + odd, NAN), grad((size_t)B * ecap + odd, NAN);
    for (int b = 0; b < B; ++b)
        if (fread(est.data() + odd + (size_t)b * ecap, 4, lens[2 * b], f) != (size_t)lens[2 * b]) return 2;
    for (int b = 0; b < B; ++b)
        if (fread(clean.data() + odd + (size_t)b * scap, 4, lens[2 * b + 1], f) != (size_t)lens[2 * b + 1]) return 2;
    fclose(f);
    const int cap = std::max(ecap, scap);
    const long long bytes = eab_stoi_workspace_bytes(B, cap), bwd_bytes = eab_stoi_bwd_workspace_bytes(B, cap);
    std::vector<double> work(bytes / 8 + 2), bwork(bwd_bytes / 8 + 2), out(2 * B);
    void* base = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(work.data()) + 15) & ~(uintptr_t)15);
    void* bbase = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(bwork.data()) + 15) & ~(uintptr_t)15);
    int rc = eab_stoi_f32(est.data() + odd, ecap, ecap, clean.data() + odd, scap, scap, lens.data(), B, base, bytes, out.data(), nullptr,
                          nullptr, nullptr, nullptr);
    if (rc) {
        printf("eab_stoi_f32 returned %d\n", rc);
        return 1;
    }
    rc = eab_stoi_bwd_f32(est.data() + odd, ecap, ecap, scap, lens.data(), B, base, bytes, fs, fe, gout.data(), 1, 1.0, bbase, bwd_bytes,
                          grad.data() + odd, ecap, nullptr);
    if (rc) {
        printf("eab_stoi_bwd_f32 returned %d\n", rc);
        return 1;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&ecap, 4, 1, o);
    fwrite(out.data(), 8, out.size(), o);
    fwrite(grad.data() + odd, 4, (size_t)B * ecap, o);
    fclose(o);
    return 0;
}
