"""float64 restatement of the contract of eab_stft_compress_bwd_f32: the adjoint of the STFT front end
``stft_compress`` -- reflect-padded, windowed one-sided DFT followed by the compression X |X|^-1/2 -- evaluated at the
forward's stored output.  Plain numpy, no device; tests/test_stft_bwd_ref.py checks it against float64 torch autograd and
tests/test_stft_bwd_gpu.py checks the kernel against it."""
import numpy as np

CASES = [(320, 160, 320), (512, 128, 400), (320, 100, 320)]      # (n_fft, hop, win_length)


def padded_window(n_fft: int, win: int) -> np.ndarray:
    """periodic Hann of ``win`` samples, zero-padded to n_fft and centred (what torch.stft does with win_length < n_fft)"""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win)
    left = (n_fft - win) // 2
    return np.pad(w, (left, n_fft - win - left))


def to_bmtf(a: np.ndarray, layout: int) -> np.ndarray:
    """(B,T,F,M,2) [layout 0] or (B,2,T,F) [layout 1] -> complex (B, M, T, F)"""
    a = np.asarray(a, dtype=np.float64)
    if layout == 0:
        return (a[..., 0] + 1j * a[..., 1]).transpose(0, 3, 1, 2)
    return (a[:, 0] + 1j * a[:, 1])[:, None]


def from_bmtf(z: np.ndarray, layout: int) -> np.ndarray:
    """complex (B, M, T, F) -> the layout's real array"""
    if layout == 0:
        return np.stack([z.real, z.imag], axis=-1).transpose(0, 2, 3, 1, 4)
    return np.stack([z[:, 0].real, z[:, 0].imag], axis=1)


def compress_grad(s: np.ndarray, g: np.ndarray) -> np.ndarray:
    """dL/dX for s = X |X|^-1/2 stored, g = dL/ds (complex arrays standing for real pairs):
    g / rho - s (s . g) / (2 rho^3) with the real dot product; exactly 0 where rho = 0"""
    rho = np.abs(s)
    dot = s.real * g.real + s.imag * g.imag
    safe = np.where(rho > 0, rho, 1.0)
    out = g / safe - s * dot / (2.0 * safe ** 3)
    return np.where(rho > 0, out, 0.0)


def stft_compress_bwd_ref(dspec, spec, window, n_fft: int, hop: int, layout: int, L: int, lengths=None) -> np.ndarray:
    """dwav (B, M, L) float64.  window: n_fft samples.  lengths: per-utterance sample counts (None: L each); frames
    t >= 1 + L_b // hop of dspec and spec are not read (they may hold NaN)."""
    g, s = to_bmtf(dspec, layout), to_bmtf(spec, layout)
    B, M, T, F = s.shape
    H = n_fft // 2
    assert F == H + 1 and T == 1 + L // hop
    w = np.asarray(window, dtype=np.float64)
    th = 2.0 * np.pi * np.outer(np.arange(F), np.arange(n_fft)) / n_fft      # [k][n]
    cosm, sinm = np.cos(th), np.sin(th)
    dwav = np.zeros((B, M, L))
    for b in range(B):
        Lb = L if lengths is None else int(lengths[b])
        Tb = 1 + Lb // hop
        gx = compress_grad(s[b, :, :Tb], g[b, :, :Tb])                        # (M, Tb, F)
        u = (gx.real @ cosm - gx.imag @ sinm) * w                             # (M, Tb, n_fft): interior bins not doubled
        dpad = np.zeros((M, Lb + 2 * H))
        for t in range(Tb):
            dpad[:, t * hop:t * hop + n_fft] += u[:, t]
        j = np.arange(Lb)
        d = dpad[:, j + H]
        head = (j >= 1) & (j <= H)
        d[:, head] = d[:, head] + dpad[:, H - j[head]]
        tail = (j >= Lb - 1 - H) & (j <= Lb - 2)
        d[:, tail] = d[:, tail] + dpad[:, 2 * (Lb - 1) - j[tail] + H]
        dwav[b, :, :Lb] = d
    return dwav
