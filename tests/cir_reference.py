"""Channel impulse response (CIR) from the phase reference symbol (Mode I) restated from the definition in numpy, for the
tests of dabgpu_cir_*: the per-frame records (window -> the TII calls' frequency correction -> float64 FFT -> tapered
inverse -> taps and carrier powers), the noise tap power of white noise, and the analysis rule.  R is built from
synth.prs_carriers(), not from the library.

Error budgets.  U = 2^-24; every budget is a forward-error bound of a correct float32 implementation of the same
operation (Higham: sums section 3.1, FFT theorem 24.2; C_FFT = 7 per radix-2 stage), with the spectral budget
E_X = (C_FFT 11 + C_nco) U ||y||_2 per bin and the direct-NCO constant C_NCO_DIRECT = 8 that tii_reference.py derives
(0 where dphi == 0).
- Carrier: 1536 / 2048^2 is exact in float32, so carrier = s |X_k|^2 moves by s (2 |X_k| E_X + E_X^2) and its own
  arithmetic (a power's gamma_2, one product) by C_CAR U s (|X_k| + E_X)^2, C_CAR = 3.
- Taper.  The weight 0.5 + 0.5 cos(pi k / 769) is formed as fma(0.5, cospi(float(k) * float(1 / 769)), 0.5): the
  argument carries 2 U relative (the rounded constant, the product), at most 2 U absolute since it stays below 1, which
  cos(pi x) turns into at most 2 pi U; cospi itself 2 ulp (2 U); halved, plus the fma's own rounding (at most U / 2 of a
  value below 1, counted as U): an ABSOLUTE error of C_TAPER U, C_TAPER = 3.2 + 1 + 1 rounded up to 6, which at the band
  edges, where the weight falls to 4e-6, is not small relative to the weight.  The scale sqrt(1536) / (2048 768)
  (rounded once), its product with the weight and the product with X add C_Y = 3 roundings relative to Y.  So, with
  Y[k] = scale w(k) X[k] conj R[k] (R a fourth root of unity: swaps and negations, exact), X_band the 1536 carriers:
    ||dY||_2 <= scale (sqrt(sum w^2) E_X + C_TAPER U ||X_band||_2) + C_Y U ||Y||_2.
- Tap: h is a second 2048-point transform of Y (unnormalised), so an input error dY reaches the taps with 2-norm
  sqrt(2048) ||dY||_2 and the transform adds C_FFT 11 U sqrt(2048) ||Y||_2; spread over the 2048 taps as E_X is over
  the bins, E_h = ||dY||_2 + C_FFT 11 U ||Y||_2 per tap, and tap = |h|^2 moves by at most
    2 sqrt(tap) E_h + E_h^2 + C_POW U (sqrt(tap) + E_h)^2,  C_POW = 2 (gamma_2 of a power).
  On a 15 dB two-path PRS the largest tap budget is 0.8 % of the 1e-4-of-the-peak bar test_cir.py used, and the median
  budget is 2e-4 of the median (noise-floor) tap, where that bar was 5 times the tap itself.
The accumulators carry no budget: a call's sum is bit for bit the sequential float32 frame-order sum of its records
added to what the accumulator held, the frame count added as an integer."""
import math

import numpy as np

from dabgpu import synth
from ofdm_reference import C_FFT, LOG2N, U
from tii_reference import C_NCO_DIRECT

C_CAR, C_TAPER, C_Y, C_POW = 3.0, 6.0, 3.0, 2.0

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


def phase_step(freq_offset):
    """dphi of correct(): 0 means the samples are left as they are."""
    f = float(np.float32(freq_offset))
    return int(round(f * 4294967296.0)) & 0xFFFFFFFF


_PRS = None


def record(window, freq_offset=0.0, budgets=False):
    """One frame: window = the 2048 samples [504, 2552) after its PRS prefix -> (tap [2048], carrier [1536]), float64, and
    with budgets=True also (tap budget [2048], carrier budget [1536])."""
    global _PRS
    if _PRS is None:
        _PRS = prs()
    y = correct(np.asarray(window).reshape(NB_FFT), freq_offset)
    X = np.fft.fft(y)
    Xk = X[BINS]
    Y = np.zeros(NB_FFT, np.complex128)
    Y[BINS] = W * Xk * np.conj(_PRS)
    scale = math.sqrt(N_CARRIERS) / (NB_FFT * S)
    h = scale * np.fft.ifft(Y) * NB_FFT                                       # sum_k Y[k] exp(+2 pi i k n / 2048)
    tap, car = np.abs(h) ** 2, N_CARRIERS / NB_FFT ** 2 * np.abs(Xk) ** 2
    if not budgets:
        return tap, car
    e_x = (C_FFT * LOG2N + (C_NCO_DIRECT if phase_step(freq_offset) else 0.0)) * U * math.sqrt(float((np.abs(y) ** 2).sum()))
    m = np.abs(Xk)
    s = N_CARRIERS / NB_FFT ** 2
    car_b = s * (2.0 * m * e_x + e_x * e_x) + C_CAR * U * s * (m + e_x) ** 2
    norm_y = scale * math.sqrt(float((np.abs(Y) ** 2).sum()))
    d_y = scale * (math.sqrt(float((W ** 2).sum())) * e_x + C_TAPER * U * math.sqrt(float((m ** 2).sum()))) + C_Y * U * norm_y
    e_h = d_y + C_FFT * LOG2N * U * norm_y
    a = np.sqrt(tap)
    tap_b = 2.0 * a * e_h + e_h * e_h + C_POW * U * (a + e_h) ** 2
    return tap, car, tap_b, car_b


def records(iq, prs_starts, freq_offsets=None, budgets=False):
    """Records of the frames whose PRS prefixes start at prs_starts in the 1-D array iq -> (tap [n][2048], carrier [n][1536]),
    with budgets=True also (tap budgets [n][2048], carrier budgets [n][1536])."""
    out = []
    for i, s in enumerate(prs_starts):
        s = int(s)
        out.append(record(iq[s + WIN_BEGIN:s + WIN_END], 0.0 if freq_offsets is None else freq_offsets[i], budgets))
    return tuple(np.array(a) for a in zip(*out))


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
