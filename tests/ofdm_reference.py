"""The Mode I OFDM front end (rows A2..A6: NCO, 2048-point FFT, DQPSK, frequency de-interleave, soft-bit quantiser)
restated from EN 300 401 and include/dabgpu.h in float64 / complex128, for the tests of dabgpu_ofdm_demod_* and
dabgpu_fft_symbols.  Written without oracle/, dab_tables.hpp, dabgpu/synth.py or the library, so that a mistake they
share cannot pass.

Definitions (frame = 76 symbols of 2552 samples, starting at the first sample of the phase reference symbol's prefix):
- NCO: the ABI quantises the correction f (the float32 the kernel receives) to a 32-bit phase step
  dphi = llrint(f 2^32) mod 2^32 (ties to even); sample n of the frame (prefix included) is multiplied by
  exp(+j 2 pi frac(n dphi / 2^32)), the phase formed in exact integer arithmetic.
- FFT: np.fft.fft of samples 504..2551 of each symbol (unnormalised, natural bin order).
- Carriers k = -768..768 without 0 sit in bins k mod 2048; d_l[k] = X_l[k] conj(X_{l-1}[k]), l = 1..75.
- Frequency de-interleave (section 14.6): PI(0) = 0, PI(i) = (13 PI(i-1) + 511) mod 2048; the values in 256..1792 other
  than 1024, in order, minus 1024, are the carriers of data indices 0..1535.
- Soft values: v = -127 c / max(|re d|, |im d|) for c = re d (bits 0..1535 of the symbol) and c = im d (bits
  1536..3071), data-index order; v = 0 where d = 0.  The soft bit is trunc(v).
- Cyclic-prefix correlation of symbol l: sum_{i<504} conj(y[i]) y[i+2048] over the symbol's corrected samples.
- dd4 (dabgpu_ofdm_demod_frames_dd_dev): entry 0 = the PRS prefix correlation; symbol l contributes sum u^4 over bins
  v + 64 m (v < 64, m in {0, 1, 30, 31}, bin 0 replaced by 768), u = d_l / |d_l| (0 where d_l = 0).  A launch cut into
  runs puts each run's total in the entry of its last symbol.

Error budgets.  u = 2^-24 (float32 unit roundoff).  Every budget is a forward-error bound of a correct float32
implementation of the same operation, built from the standard bounds (Higham, "Accuracy and Stability of Numerical
Algorithms", 2nd ed.: sums and dot products section 3.1, FFT theorem 24.2), with these constants:
- C_FFT = 7 per radix-2 stage: theorem 24.2 gives eta = mu + gamma_4 (sqrt 2 + mu) ~ 6.7 u per stage for twiddles
  rounded once from float64 (mu <= u); radix-16 and radix-8 stages round no more often than the radix-2 stages they
  replace, so 7 u log2(2048) bounds the spectrum's relative 2-norm error.
- C_NCO = 128: a correction adds a relative error per sample of at most 1.6 u from the phase's 24-bit mantissa
  (float(int32 phase): 2^-26 of a turn), 2.9 u from sincospif (2 ulp per component), and, because the per-lane phasor
  is rotated by r128 up to 15 times, 15 x (4.5 u for r128's own two errors + 3 u per complex product); codd[]'s extra
  sample period adds 7.5 u.  That is 125 u; dphi = 0 makes every phasor exactly 1 (C_NCO = 0).
- Both are 2-norm bounds of the whole symbol; spread over its 2048 bins (Parseval) they give the per-bin budget
  E_l = (C_FFT log2 N + C_NCO) u ||y_l||_2, y_l the symbol's 2048 corrected samples -- the root mean square a worst-case
  rounding could reach in every bin.  Per-bin errors of real rounding are uncorrelated and a log2 N growth is already
  sqrt(log2 N) times the statistical one, so a single bin exceeds E_l only with a many-sigma excursion.
- Soft values: with r = E_l / |X_l[k]| + E_{l-1} / |X_{l-1}[k]| + r_l r_{l-1} + 4 u (the product d's rounding),
  |delta d| / |d| <= r; since |c| <= A, |delta A| <= |delta d| and A >= |d| / sqrt 2, |delta v| <= 127 2 sqrt 2 r.
  C_Q = 8 adds the quantiser's own arithmetic: the 1-ulp v_rcp and its product (2 u) and the 2^-22 head-room of
  -127.00003 (4 u), rounded up.  The band is eps_k = 127 (2 sqrt 2 r + C_Q u) LSB; a soft bit may differ from trunc(v)
  only where v lies within eps_k of a point where trunc jumps (a non-zero integer).
- Constellation: |delta d| <= E_l |X_{l-1}| + |X_l| E_{l-1} + E_l E_{l-1} + 4 u |X_l| |X_{l-1}|.
- Cyclic-prefix correlations: C_CYC = 32 times u sum |y[i]| |y[i+2048]|: a 504-term dot product summed as 16 terms per
  lane and a six-level wave reduction (gamma_22), then rotated by a phasor carrying 4.5 u, rounded up.
- dd4: a term u^4 moves by at most 4 |delta u| <= 4 (2 |delta d| / |d| + C_U u), C_U = 8 for the unit vector's rsq and
  the two squarings; a run's sum adds gamma_(10 + symbols in the run) times its number of terms (four terms per lane,
  the wave reduction, one addition per symbol).
"""
import numpy as np

NB_FFT, NB_CP, NB_SYM, NB_SYMBOLS, NB_CARRIERS = 2048, 504, 2552, 76, 1536
NB_DATA_SYMBOLS = NB_SYMBOLS - 1
NB_SYM_BITS = 2 * NB_CARRIERS
NB_FRAME_BITS = NB_DATA_SYMBOLS * NB_SYM_BITS
FRAME_SAMPLES = NB_SYMBOLS * NB_SYM
LOG2N = 11

U = 2.0 ** -24
C_FFT, C_NCO, C_Q, C_CYC, C_U = 7.0, 128.0, 8.0, 32.0, 8.0


# ------------------------------------------------------------------------------------------------------------- tables
def deinterleave_carriers():
    """Carrier k (-768..768, not 0) of data index n = 0..1535, from the section 14.6 recurrence."""
    pi = [0]
    for _ in range(1, NB_FFT):
        pi.append((13 * pi[-1] + 511) % NB_FFT)
    return np.array([p - 1024 for p in pi if 256 <= p <= 1792 and p != 1024], np.int64)


CARRIERS = deinterleave_carriers()
DATA_BINS = CARRIERS % NB_FFT                      # bin of data index n
ORDER_BINS = np.concatenate([np.arange(-768, 0), np.arange(1, 769)]) % NB_FFT   # bin of carrier-order index -768..768
DD_BINS = np.concatenate([np.arange(128), np.arange(1920, 2048)])
DD_BINS[0] = 768


def dphi_of(f):
    """The 32-bit phase step the ABI applies for the float32 correction f (cycles/sample)."""
    return int(np.rint(np.float64(np.float32(f)) * 4294967296.0)) % (1 << 32)


def stream_correction(fine, coarse):
    """The float32 correction a closed-loop call applies: fine + coarse added in float32 (csrc/ofdm_kernels.hip)."""
    return np.float32(np.float32(fine) + np.float32(coarse))


def nco(n_samples, dphi):
    n = np.arange(n_samples, dtype=np.int64)
    ph = (n * np.int64(dphi)) & 0xFFFFFFFF
    return np.exp(2j * np.pi * (ph.astype(np.float64) / 4294967296.0))


def cu8_values(u):
    """cu8 samples: u - 127.5 (csrc/iq_load.hpp)."""
    return np.asarray(u, np.float64) - 127.5


# ---------------------------------------------------------------------------------------------------------- the front end
class Frame:
    """One frame through the reference.  x: 76 * 2552 complex samples (any dtype; integer formats as their values), f:
    the float32 correction (or dphi: the phase step itself).  Attributes (float64 / complex128):
      X [76][2048] spectra, E [76] per-bin spectral budget
      d [75][1536] differential symbols (data-index order), v [230400] soft values, eps [230400] their band (LSB),
      A [75][1536] max(|re d|, |im d|)
      cyc [76] cyclic-prefix correlations, cyc_budget [76]
    Methods: dqpsk() (carrier order, with its budget), dd4_terms() (per-symbol sums and budgets)."""

    def __init__(self, x, f=0.0, dphi=None):
        x = np.asarray(x).astype(np.complex128).reshape(-1)
        assert x.size >= FRAME_SAMPLES
        x = x[:FRAME_SAMPLES]
        self.dphi = dphi_of(f) if dphi is None else int(dphi) % (1 << 32)
        y = x * nco(FRAME_SAMPLES, self.dphi) if self.dphi else x
        sym = y.reshape(NB_SYMBOLS, NB_SYM)
        useful = sym[:, NB_CP:]
        self.X = np.fft.fft(useful, axis=1)
        c = C_FFT * LOG2N + (C_NCO if self.dphi else 0.0)
        self.E = c * U * np.sqrt((np.abs(useful) ** 2).sum(axis=1))
        # cyclic-prefix correlations
        head, tail = sym[:, :NB_CP], sym[:, NB_FFT:]
        self.cyc = (np.conj(head) * tail).sum(axis=1)
        self.cyc_budget = C_CYC * U * (np.abs(head) * np.abs(tail)).sum(axis=1)
        # DQPSK and soft values
        Xd = self.X[:, DATA_BINS]
        self.d = Xd[1:] * np.conj(Xd[:-1])
        self.A = np.maximum(np.abs(self.d.real), np.abs(self.d.imag))
        ok = self.A > 0
        safe = np.where(ok, self.A, 1.0)
        vr = np.where(ok, -127.0 * (self.d.real / safe), 0.0)      # (|c| = A gives exactly -+127)
        vi = np.where(ok, -127.0 * (self.d.imag / safe), 0.0)
        self.v = np.concatenate([vr, vi], axis=1).reshape(-1)
        self.r = self._rel_error(Xd)
        eps = 127.0 * (2.0 * np.sqrt(2.0) * self.r + C_Q * U)
        self.eps = np.concatenate([eps, eps], axis=1).reshape(-1)

    def _rel_error(self, Xm):
        """r = relative error bound of d per data symbol and carrier (inf where a spectrum value is 0)."""
        mag = np.abs(Xm)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(mag > 0, self.E[:, None] / np.where(mag > 0, mag, 1.0), np.inf)
        return rel[1:] + rel[:-1] + rel[1:] * rel[:-1] + 4.0 * U

    # --- derived views
    def soft(self):
        """The exact soft bits trunc(v), int8 [230400]."""
        return np.trunc(self.v).astype(np.int8)

    def edge_distance(self):
        """Distance of every v from the nearest point where trunc jumps (the non-zero integers)."""
        a = np.abs(self.v)
        return np.where(a < 0.5, 1.0 - a, np.abs(a - np.rint(a)))

    def in_band(self):
        return self.edge_distance() <= self.eps

    def larger_component(self):
        """[230400] bool: the bit is the larger component of its carrier by more than the band (its soft bit must be
        +-127 exactly); erased carriers (A == 0) are excluded."""
        re = np.abs(self.d.real)
        im = np.abs(self.d.imag)
        live = self.A > 0
        gap = np.where(live, np.where(live, self.A, 0.0) * np.where(live, self.r * 2.0 * np.sqrt(2.0) + C_Q * U, 0.0), 0.0)
        big_re = (re - im > gap) & live
        big_im = (im - re > gap) & live
        return np.concatenate([big_re, big_im], axis=1).reshape(-1)

    def erased(self):
        """[75][1536] bool: carriers with d == 0."""
        return self.A == 0

    def dqpsk(self):
        """(d in carrier order -768..768 [75][1536], per-element budget)."""
        Xo = self.X[:, ORDER_BINS]
        d = Xo[1:] * np.conj(Xo[:-1])
        m = np.abs(Xo)
        e = self.E[:, None]
        budget = e[1:] * m[:-1] + m[1:] * e[:-1] + e[1:] * e[:-1] + 4.0 * U * m[1:] * m[:-1]
        return d, budget

    def dd4_terms(self):
        """(t [76], b [76]): t[l] = sum over the dd bins of u_l^4 for l = 1..75, t[0] = the PRS prefix correlation;
        b[l] = that sum's term budget (b[0]: the correlation's)."""
        Xb = self.X[:, DD_BINS]
        d = Xb[1:] * np.conj(Xb[:-1])
        mag = np.abs(d)
        unit = np.where(mag > 0, d / np.where(mag > 0, mag, 1.0), 0.0)
        t = np.zeros(NB_SYMBOLS, np.complex128)
        b = np.zeros(NB_SYMBOLS)
        t[1:] = (unit ** 4).sum(axis=1)
        b[1:] = (4.0 * np.minimum(2.0 * self._rel_error(Xb) + C_U * U, 2.0)).sum(axis=1)
        t[0], b[0] = self.cyc[0], self.cyc_budget[0]
        return t, b


def run_bounds(parts):
    """Data-symbol runs (l_first, l_last] of a frame cut into `parts` runs, as the launch cuts them."""
    return [(NB_DATA_SYMBOLS * p // parts, NB_DATA_SYMBOLS * (p + 1) // parts) for p in range(parts)]


def dd4_expected(fr, parts=1):
    """(entries [76], budget [76]) of a frame cut into `parts` runs: each run's sum in the entry of its last symbol, 0 in
    its other entries (budget 0: they must be exactly 0)."""
    t, b = fr.dd4_terms()
    out = np.zeros(NB_SYMBOLS, np.complex128)
    bud = np.zeros(NB_SYMBOLS)
    out[0], bud[0] = t[0], b[0]
    for lo, hi in run_bounds(parts):
        out[hi] = t[lo + 1:hi + 1].sum()
        n_terms = 256 * (hi - lo)
        bud[hi] = b[lo + 1:hi + 1].sum() + (10 + (hi - lo)) * U * n_terms
    return out, bud
