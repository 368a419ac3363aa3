    // The body of istft_kernel<VARLEN> (LIN = false) and istft_lin_kernel<VARLEN> (LIN = true), included by istft.hip inside each
    // kernel: see the comment above them.
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int NH = n_fft / 2, F = NH + 1;
    const int R = (n_fft + hop - 1) / hop;                        // most frames that cover one output sample (2 for the reference)
    float2* tw = reinterpret_cast<float2*>(smem);                 // [n_fft] exp(-2 pi i j / n_fft)
    float2* buf0 = tw + n_fft;                                    // [FFT_SIGS][NH]
    float2* buf1 = buf0 + FFT_SIGS * NH;
    float* win = reinterpret_cast<float*>(buf1 + FFT_SIGS * NH);  // [n_fft]
    float* xs = win + n_fft;                                      // [FFT_SIGS][2][F] staged spectrum rows
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int t0 = chunk * (FFT_SIGS - (R - 1));                  // consecutive workgroups share R-1 frames
    const int Tb = VARLEN ? (lens[b] > T ? T : (lens[b] < 1 ? 1 : lens[b])) : T;   // frames of this utterance
    if (VARLEN && t0 >= Tb) {
        // every frame of this workgroup lies past the utterance (workgroup-uniform, before any barrier): its positions
        // start at t0 hop + n_fft - hop - n_fft/2 >= hop (Tb - 1), all of them padding -- zeros, no transform
        const int p0 = t0 * hop + n_fft - hop, p1 = p0 + (FFT_SIGS - (R - 1)) * hop, cap_len = hop * (T - 1);
        for (int p = p0 + tid; p < p1; p += ISTFT_THREADS) {
            const int j = p - NH;
            if (j >= 0 && j < cap_len) wav[(size_t)b * cap_len + j] = 0.0f;
        }
        return;
    }

    for (int k = tid; k < n_fft; k += ISTFT_THREADS) {
        const float2 cs = reinterpret_cast<const float2*>(twiddle)[k];     // (cos, sin)(+theta)
        tw[k] = make_float2(cs.x, -cs.y);
        win[k] = window[k];
    }
    // stage re/im rows of the frames (coalesced; the split below reads them mirrored)
    for (int e = tid; e < FFT_SIGS * 2 * F; e += ISTFT_THREADS) {
        const int c = e / (2 * F), r = e - c * 2 * F;
        const int ri = r / F, f = r - ri * F;
        const int t = t0 + c;
        xs[e] = t < Tb ? spec[(((size_t)b * 2 + ri) * T + t) * F + f] : 0.0f;
    }
    __syncthreads();
    // conj(Z[k]),  Z = E + iO
    for (int e = tid; e < FFT_SIGS * NH; e += ISTFT_THREADS) {
        const int c = e / NH, k = e - c * NH;
        const float* re = xs + c * 2 * F;
        const float* im = re + F;
        float2 xk = make_float2(re[k], im[k]);
        float2 xm = make_float2(re[NH - k], im[NH - k]);
        if (LIN) {
            xk = istft_decompress(xk);
            xm = istft_decompress(xm);
        }
        if (k == 0) xk.y = xm.y = 0.0f;                            // C2R: DC and Nyquist are real
        const float2 E = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
        const float2 D = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
        const float2 O = cmul(D, make_float2(tw[k].x, -tw[k].y)); // * e^{+i theta_k}
        buf0[e] = make_float2(E.x - O.y, -(E.y + O.x));
    }
    __syncthreads();
    const float2* y = fft_run(buf0, buf1, tw, NH, n_fft, plan, tid, ISTFT_THREADS);
    // x_c[2j] = Re y_c[j] / NH,  x_c[2j+1] = -Im y_c[j] / NH
    const float inv = 1.0f / (float)NH;
    const float* yf = reinterpret_cast<const float*>(y);
    // Overlap-add over the frames that cover a sample, divided by the squared-window envelope of the frames that exist
    // (torch.istft), then the centre trim.  This workgroup holds frames t0 .. t0+7 and emits the padded positions
    // [p_lo, p_hi) whose covering frames it holds completely (the first workgroup: from 0); highest frame first.
    const int per = FFT_SIGS - (R - 1);
    const int p_lo = chunk == 0 ? 0 : t0 * hop + n_fft - hop;
    const int p_hi = (t0 + per) * hop + n_fft - hop;
    const int out_len = hop * (T - 1), len_b = hop * (Tb - 1);     // row stride of wav; samples of this utterance
    for (int e = tid; e < p_hi - p_lo; e += ISTFT_THREADS) {
        const int p = p_lo + e;
        const int j = p - NH;                                      // output sample (centre trim of n_fft/2)
        if (j < 0 || j >= out_len) continue;
        if (VARLEN && j >= len_b) {                                // past the utterance's trim: zero
            wav[(size_t)b * out_len + j] = 0.0f;
            continue;
        }
        const int th = p / hop;
        float acc = 0.0f, env = 0.0f;
        for (int r = 0; r < R; ++r) {
            const int t = th - r;
            const int idx = p - t * hop;                           // sample of frame t; float index = idx (re/im interleave)
            if (t < 0 || idx >= n_fft) break;
            if (t >= Tb) continue;
            float a = yf[(t - t0) * n_fft + idx];
            if (idx & 1) a = -a;
            const float w = win[idx];
            acc = fmaf(w, a * inv, acc);
            env = fmaf(w, w, env);
        }
        wav[(size_t)b * out_len + j] = acc / env;
    }
