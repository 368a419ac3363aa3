// Stand-alone driver of the host emulation of csrc/stoi.hip: eab_stoi_f32 on rows allocated at their exact size (the batch's last
// row ends where its allocation ends) and poisoned with NaN past every utterance's own length, so that AddressSanitizer sees a
// read past a row and the scores see a read past a length.
//   stoi_emulation IN OUT UNALIGNED TAPS
// IN:  int32 B, B x (int32 est samples, int32 clean samples), the est rows, the clean rows (fp32, own lengths, back to back)
// OUT: int32 FC, double [B][2] scores, int32 [B] K, int32 [B][FC] kept, float [B][2][15][FC] band values
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eabnet_hip.h"

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int B = 0;
    if (fread(&B, 4, 1, f) != 1 || B < 1) return 2;
    std::vector<int> lens(2 * B);
    if (fread(lens.data(), 4, 2 * B, f) != (size_t)(2 * B)) return 2;
    int ecap = 0, scap = 0;
    for (int b = 0; b < B; ++b) {
        ecap = std::max(ecap, lens[2 * b]);
        scap = std::max(scap, lens[2 * b + 1]);
    }
    const int odd = atoi(argv[3]), taps = atoi(argv[4]);              // odd: the rows start 4 bytes past a 16-byte boundary
    std::vector<float> est((size_t)B * ecap + odd, NAN), clean((size_t)B * scap + odd, NAN);
    for (int b = 0; b < B; ++b)
        if (fread(est.data() + odd + (size_t)b * ecap, 4, lens[2 * b], f) != (size_t)lens[2 * b]) return 2;
    for (int b = 0; b < B; ++b)
        if (fread(clean.data() + odd + (size_t)b * scap, 4, lens[2 * b + 1], f) != (size_t)lens[2 * b + 1]) return 2;
    fclose(f);
    const int cap = std::max(ecap, scap), FC = eab_stoi_frame_capacity(cap);
    const long long bytes = eab_stoi_workspace_bytes(B, cap);
    std::vector<double> work(bytes / 8 + 2), out(2 * B);
    void* base = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(work.data()) + 15) & ~(uintptr_t)15);
    std::vector<int> K(B), kept((size_t)B * FC);
    std::vector<float> tob((size_t)B * 30 * FC);
    const int rc = eab_stoi_f32(est.data() + odd, ecap, ecap, clean.data() + odd, scap, scap, lens.data(), B, base, bytes, out.data(),
                                taps ? K.data() : nullptr, taps ? kept.data() : nullptr, taps ? tob.data() : nullptr, nullptr);
    if (rc) {
        printf("eab_stoi_f32 returned %d\n", rc);
        return 1;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&FC, 4, 1, o);
    fwrite(out.data(), 8, out.size(), o);
    fwrite(K.data(), 4, K.size(), o);
    fwrite(kept.data(), 4, kept.size(), o);
    fwrite(tob.data(), 4, tob.size(), o);
    fclose(o);
    return 0;
}
