"""Channel impulse response (CIR) from the phase reference symbol (Mode I) restated from the definition in numpy, for the
tests of dabgpu_cir_*: the per-frame records (window -> the TII calls' frequency correction -> float64 FFT -> tapered
inverse -> taps and carrier powers), the noise tap power of white noise, and the analysis rule.  R is built from
synth.prs_carriers(), not from the library."""
import math

import numpy as np

from dabgpu import synth

NB_FFT = 2048
N_CARRIERS = 1536
WIN_BEGIN, WIN_END = 504, 2552          # window [504, 2552) relative to the PRS prefix
GUARD = 504

K = np.array([k for k in range(-768, 769) if k != 0])          # carrier order of the `carrier` record: -768..-1, 1..768
BINS = K % NB_FFT
W = 0.5 + 0.5 * np.cos(np.pi * K / 769.0)                        # Hann taper over the band
S = W.sum()                                                      # = 768


def prs():
    """R[k] on the 1536 carriers, in K order (unit magnitude)."""
    z = synth.prs_carriers()
    return z[K + 768].astype(np.complex128)


def correct(window, freq_offset):
    """The TII calls' correction: nco(n, dphi), dphi = round(f 2^32) wrapped to 32 bits, n from the window start; the
    phase of sample n is the signed 32-bit n * dphi in units of 2^-32 cycles.  f is taken as the float32 the device holds."""
    x = np.asarray(window, np.complex128)
    f = float(np.float32(freq_offset))
    if f == 0.0:
        return x
    dphi = int(round(f * 4294967296.0)) & 0xFFFFFFFF
    ph = (np.arange(NB_FFT, dtype=np.uint64) * np.uint64(dphi)) & np.uint64(0xFFFFFFFF)
    ph = ph.astype(np.int64)
    ph = np.where(ph >= 1 << 31, ph - (1 << 32), ph)
    return x * np.exp(2j * np.pi * ph / 4294967296.0)


def record(window, freq_offset=0.0):
    """One frame: window = the 2048 samples [504, 2552) after its PRS prefix -> (tap [2048], carrier [1536]), float64."""
    X = np.fft.fft(correct(window, freq_offset))
    Xk = X[BINS]
    Y = np.zeros(NB_FFT, np.complex128)
    Y[BINS] = W * Xk * np.conj(prs())
    h = math.sqrt(N_CARRIERS) / (NB_FFT * S) * np.fft.ifft(Y) * NB_FFT        # sum_k Y[k] exp(+2 pi i k n / 2048)
    return np.abs(h) ** 2, N_CARRIERS / NB_FFT ** 2 * np.abs(Xk) ** 2


def records(iq, prs_starts, freq_offsets=None):
    """Records of the frames whose PRS prefixes start at prs_starts in the 1-D array iq -> (tap [n][2048], carrier [n][1536])."""
    taps, cars = [], []
    for i, s in enumerate(prs_starts):
        s = int(s)
        t, c = record(iq[s + WIN_BEGIN:s + WIN_END], 0.0 if freq_offsets is None else freq_offsets[i])
        taps.append(t)
        cars.append(c)
    return np.array(taps), np.array(cars)


def noise_tap_power(sigma2):
    """E|h[n]|^2 of complex white noise of variance sigma2 per sample: each bin carries 2048 sigma2, the taper and the
    scale of h keep 1536 sum(w^2) sigma2 / (2048 S^2) of it."""
    return N_CARRIERS * float((W ** 2).sum()) * sigma2 / (NB_FFT * S * S)


def median_of_mean_exponentials(frames):
    """m(F): the median of a mean of F unit exponentials (to second order in 1/F)."""
    F = float(frames)
    return 1.0 - 1.0 / (3.0 * F) + 8.0 / (405.0 * F * F)


def analyse(tap, frames, min_snr_db=10.0, range_db=25.0):
    """The analysis rule on a summed record -> (report dict, [(delay, level_db, snr_db, beyond_guard)] by delay).  tap is
    taken as the float32 the accumulator holds, the cfg values as the float32 the C struct holds; the rest is float64."""
    report = {"frames": int(frames), "n_paths": 0, "floor": 0.0, "peak": 0.0, "first_delay": 0.0, "strongest_delay": 0.0,
              "rms_delay_spread": 0.0, "guard_ratio_db": 0.0}
    if frames == 0:
        return report, []
    p = np.asarray(tap, np.float32).astype(np.float64) / float(frames)
    srt = np.sort(p)
    floor = 0.5 * (srt[1023] + srt[1024]) / median_of_mean_exponentials(frames)
    peak = srt[-1]
    report["floor"], report["peak"] = floor, peak
    if not floor > 0.0:
        return report, []
    min_snr = float(np.float32(min_snr_db))
    rng = float(np.float32(range_db))
    paths = []
    for n in range(NB_FFT):
        pm, p0, pp = p[(n - 1) % NB_FFT], p[n], p[(n + 1) % NB_FFT]
        if not (p0 > pm and p0 >= pp and p0 >= floor * 10.0 ** (min_snr / 10.0) and p0 >= peak * 10.0 ** (-rng / 10.0)):
            continue
        L = [10.0 * math.log10(max(v, 1e-30)) for v in (pm, p0, pp)]
        den = L[0] - 2.0 * L[1] + L[2]
        frac = 0.5 * (L[0] - L[2]) / den if den < 0.0 else 0.0
        paths.append((float(n - NB_FFT if n >= NB_FFT // 2 else n) + frac, p0))
    paths.sort(key=lambda t: t[0])
    if not paths:
        return report, []
    first = paths[0][0]
    strongest = max(paths, key=lambda t: t[1])[0]        # (max keeps the earliest of equal powers)
    P = np.array([q for _, q in paths])
    D = np.array([d for d, _ in paths])
    spread = 0.0
    if len(paths) > 1:
        mean = (P * D).sum() / P.sum()
        spread = math.sqrt((P * (D - mean) ** 2).sum() / P.sum())
    beyond = D - first > GUARD
    within_p, beyond_p = P[~beyond].sum(), P[beyond].sum()
    report.update(n_paths=len(paths), first_delay=first, strongest_delay=strongest, rms_delay_spread=spread,
                  guard_ratio_db=10.0 * math.log10(within_p / beyond_p) if beyond_p > 0 else math.inf)
    return report, [(d, 10.0 * math.log10(q / peak), 10.0 * math.log10(q / floor), bool(d - first > GUARD)) for d, q in paths]
