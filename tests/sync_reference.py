"""Frame synchronisation and acquisition restated from include/dabgpu.h (dabgpu_sync_result,
dabgpu_acquire_cfg, dabgpu_acquired_frame) and the definitions documented in oracle/dab_oracle.h, in float64 /
complex128, for the tests of dabgpu_sync_prs* and dabgpu_acquire*.  Written without oracle/, dab_tables.hpp or the
library; R, the PRS carriers, comes from synth.prs_carriers().

Definitions (window = 2552 samples from the candidate first sample of the PRS cyclic prefix):
- NCO: the correction f (the float32 the call receives) becomes dphi = llrint(f 2^32) mod 2^32 (ofdm_reference.dphi_of);
  sample n of [504, 2552) is multiplied by exp(+j 2 pi frac(n dphi / 2^32)), n = 0 at sample 504.
- X = FFT(corrected samples 504..2551); Q[b] = X[b+1] conj X[b]; S[b] = R[b+1] conj R[b] where bins b and b+1 are both
  carriers, else 0 (the pair across DC is not one).
- D_k = sum_b Q[(b + k) mod 2048] conj S[b] (direct sum, circular in b).  k^ = argmax |D_k|^2 over |k| <= max_coarse,
  the first maximum scanning from -max_coarse; coarse_peak_to_mean = |D_k^|^2 / mean over the 2 max_coarse + 1 values.
  max_coarse = 0: k^ = 0.
- h = IFFT(Z), Z[b] = X[(b + k^) mod 2048] conj R[b] on carriers, 0 elsewhere; tap n has the signed offset t(n) = n for
  n < 1024, n - 2048 for n >= 1024 (n = 1024 is -1024).  score[n] = |h[n]|^2 w^2, w = 1 - (1 - p) |t(n) - expected| /
  2552; the peak is the first maximum of the score; peak_to_mean = |h[peak]|^2 / mean |h|^2.  first_path_rel > 0: the
  EARLIEST tap within 504 before the peak (d = 504 .. 1) with |h|^2 >= max(rel |h[peak]|^2, 16 mean) replaces it.
- A window whose sums are zero (all |D_k|^2 = 0, all |h|^2 = 0: an all-zero window) gives k = 0, tap 0, ratios 0.
- Block L1 norm of block b: sum over its 64 samples of |re| + |im|.  avg = mean over the whole blocks; level_chunk > 0:
  chunk means (the partial last chunk over its own blocks), the level from block c * chunk on = the mean of the chunk
  means c-2 .. c+2 that exist.  ts = thr_start * level, te = thr_end * level, formed from the cfg's float32 values.
- Dip machine: a dip begins at the first block with l1 < ts and ends at the first later block e with l1 > te; it is a
  null symbol when min_blocks <= e - begin <= 83.  Its candidate is e 64 - 48, kept when >= 0 and when the frame plus
  512 samples of slack lies inside the capture; at most max_out candidates.
- Acquired frame of candidate c: fine = -angle(sum_{i=64}^{439} conj x[c+i] x[c+i+2048]) / (2 pi 2048) (float32), the
  PRS sync of x[c:] under fine, start = c + toff - margin, freq_offset = float32(fine - k^/2048), flags bit 0 =
  peak_to_mean >= min_peak_to_mean, bit 1 = 0 <= start and start + 76 2552 <= n_samples.

Error budgets.  u = 2^-24.  Each is a forward-error bound of a correct float32 implementation of the same operation,
from the standard bounds (Higham, 2nd ed.: sums and dot products section 3.1, gamma_n = n u / (1 - n u); FFT theorem
24.2) and ofdm_reference's constants C_FFT = 7 per radix-2 stage, C_NCO = 128 (0 for dphi = 0).  Like ofdm_reference, a
2-norm bound of a transform's output spread over its N = 2048 elements (Parseval) is the per-element budget.
- X: E = (C_FFT log2 N + C_NCO) u ||y||_2 per bin (y the 2048 corrected samples).
- Q: dQ[b] = E (|X[b]| + |X[b+1]|) + E^2 + 4 u |X[b]| |X[b+1]| (the complex product's rounding).
- D_k, per element, the larger of the two ways a correct implementation forms it:
  direct sum (S[b] is a power of j: additions only): gamma_1535 sum |Q| + sum dQ over the 1535 pairs;
  FFT correlation (IFFT(FFT(Q) conj FFT(S)), FFT(S) a float32 table, P = max |FFT(S)|): P / sqrt(N) (||dQ||_2 +
  (2 C_FFT log2 N + 6) u ||Q||_2) -- two transforms, the table's rounding (sqrt 2 u) and the product (4 u).
- |D_k|^2: d2 = 2 |D_k| dD + dD^2 + 3 u |D_k|^2.
- coarse_peak_to_mean, relative: d2[k] / |D_k|^2 + sum d2 / sum |D|^2 + gamma_(2 max + 1) + 2 u (two divisions).
- h, per tap: dh = (sqrt(1536) E + C_FFT log2 N u ||Z||_2) / N (the input error of 1536 carriers through the inverse
  transform, plus its own); |h|^2: dM = 2 |h| dh + dh^2 + 3 u |h|^2; mean: (sum dM + gamma_N sum M) / N + u mean.
- score: w in float32 (decay = (1 - p) (1/2552), three roundings, times |t - e|, one more, 1 - that, one more) carries
  dw <= 5 u; dscore = dM w^2 + M (2 w dw + dw^2) + 2 u M w^2.
- peak_to_mean, relative: dM[peak] / M[peak] + dmean / mean + u.
- first-path threshold: dthr = max(rel dM[peak] + 2 u rel M[peak], 16 dmean + u 16 mean).
- block L1 norms: gamma_127 l1 (128 terms in any order); the level: 129 u level (the norms' error, the float32 result and
  the product with the threshold are 127 + 1 + 1 u; the double accumulation is below one u).
- the cyclic-prefix sum c = sum conj x[i] x[i+2048]: dc = 4 u sum |x[i]| |x[i+2048]| (two products and a sum per term
  in float32, the sum in float64); its angle: dtheta = asin(min(1, dc / |c|)); fine: dtheta / (2 pi 2048) + 2 u |fine|
  (the reference rounds fine to float32 as the implementation does: half an ulp each).
  freq_offset: dfine + u (|fine| + |k|/2048) (the float32 difference).

No budget comes out above the 1e-3 that test_sync.py allows against the oracle: the ratios' largest term is
gamma_(2 max + 1) <= gamma_2047 = 1.2e-4, which a sequential float32 sum (the oracle's) needs.

Acceptance ("indistinguishable set").  An integer choice i (k^, the peak, the first-path tap, a dip decision) is
accepted when s_i + d_i >= max_j (s_j - d_j); the case is UNAMBIGUOUS when that set holds one element, and then only
exact equality passes.  Threshold decisions are exact unless the reference value lies within its band of the threshold.
Where the cyclic-prefix angle lies within its band of +-pi either branch is accepted, each with its own k^ and tap."""
import itertools
import math

import numpy as np

from dabgpu import synth
from ofdm_reference import C_FFT, C_NCO, LOG2N, U, dphi_of

N = 2048
NB_CP = 504
NB_SYM = 2552
FRAME_LEN = 76 * NB_SYM
MAX_DIP_BLOCKS = 2 * 2656 // 64                                  # 83
CP_FIRST, CP_LAST = 64, 440                                      # prefix samples of the fine estimate


def gamma(n):
    return n * U / (1.0 - n * U)


def _tables():
    z = synth.prs_carriers()
    R = np.zeros(N, np.complex128)
    for k in range(-768, 769):
        if k:
            R[k % N] = z[k + 768]
    car = R != 0
    S = np.zeros(N, np.complex128)
    pair = car & np.roll(car, -1)
    pair[N - 1] = False                                          # (bin 0 is not a carrier anyway)
    S[pair] = np.roll(R, -1)[pair] * np.conj(R[pair])
    return R, car, S, np.flatnonzero(pair)


R, CARRIER, S, PAIRS = _tables()
P_MAX = float(np.abs(np.fft.fft(S)).max())
T_OF = np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N)     # signed offset of tap n


def signed_tap(n):
    return int(T_OF[int(n) % N])


def nco(dphi, n0=0, n=N):
    ph = ((np.arange(n0, n0 + n, dtype=np.int64) * np.int64(dphi)) & 0xFFFFFFFF).astype(np.float64)
    return np.exp(2j * np.pi * ph / 4294967296.0)


def coarse_direct(Q, max_coarse):
    """D_k, k = -max .. max, as the direct sum (the definition)."""
    ks = np.arange(-max_coarse, max_coarse + 1)
    idx = (PAIRS[None, :] + ks[:, None]) % N
    return (Q[idx] * np.conj(S[PAIRS])[None, :]).sum(axis=1)


def coarse_fft(Q, max_coarse):
    """The same by a float64 circular correlation (Q may be [..., N])."""
    D = np.fft.ifft(np.fft.fft(Q, axis=-1) * np.conj(np.fft.fft(S)), axis=-1)
    ks = np.arange(-max_coarse, max_coarse + 1) % N
    return D[..., ks]


def indistinguishable(s, d):
    """Indices i with s_i + d_i >= max_j (s_j - d_j)."""
    return np.flatnonzero(s + d >= (s - d).max())


class Sync:
    """The PRS sync of one window.  window: >= 2552 samples (any dtype; integer formats as their values).  f: the float32
    correction, or dphi.  D (optional): precomputed D_k (coarse_fft of a batch).  Attributes: k (the reference's k^),
    k_set, D2, d2, cptm, cptm_rel; taps(k) -> the tap analysis for coarse offset k."""

    def __init__(self, window, f=0.0, max_coarse=200, expected=0, distance_prob=1.0, first_path_rel=0.0, dphi=None, D=None):
        x = np.asarray(window).astype(np.complex128).reshape(-1)[NB_CP:NB_SYM]
        self.dphi = dphi_of(f) if dphi is None else int(dphi) % (1 << 32)
        self.y = x * nco(self.dphi) if self.dphi else x
        self.X = np.fft.fft(self.y)
        self.max_coarse = int(max_coarse)
        self.expected = int(expected)
        self.p = float(np.float32(distance_prob))
        self.rel = float(np.float32(first_path_rel))
        self.E = (C_FFT * LOG2N + (C_NCO if self.dphi else 0.0)) * U * math.sqrt(float((np.abs(self.y) ** 2).sum()))
        X, E = self.X, self.E
        X1 = np.roll(X, -1)
        self.Q = X1 * np.conj(X)
        dQ = E * (np.abs(X) + np.abs(X1)) + E * E + 4.0 * U * np.abs(X) * np.abs(X1)
        self.D = coarse_direct(self.Q, self.max_coarse) if D is None else np.asarray(D)
        dD_direct = gamma(len(PAIRS)) * np.abs(self.Q[PAIRS]).sum() + dQ[PAIRS].sum()
        dD_fft = P_MAX / math.sqrt(N) * (math.sqrt((dQ ** 2).sum()) +
                                         (2 * C_FFT * LOG2N + 6) * U * math.sqrt((np.abs(self.Q) ** 2).sum()))
        self.dD = max(dD_direct, dD_fft)
        a = np.abs(self.D)
        self.D2 = a ** 2
        self.d2 = 2 * a * self.dD + self.dD ** 2 + 3 * U * self.D2
        tot = self.D2.sum()
        if tot > 0:
            i = int(np.argmax(self.D2))                          # (numpy: the first maximum)
            self.k = i - self.max_coarse
            self.k_set = set(int(j) - self.max_coarse for j in indistinguishable(self.D2, self.d2))
            self.cptm_rel = lambda k: (self.d2[k + self.max_coarse] / self.D2[k + self.max_coarse] + self.d2.sum() / tot +
                                       gamma(2 * self.max_coarse + 1) + 2 * U)
            self.cptm_of = lambda k: self.D2[k + self.max_coarse] / (tot / self.D2.size)
        else:
            self.k, self.k_set = 0, {0}
            self.cptm_rel = lambda k: 0.0
            self.cptm_of = lambda k: 0.0
        self.cptm = self.cptm_of(self.k)
        self._taps = {}

    @property
    def unambiguous(self):
        return len(self.k_set) == 1 and self.taps(self.k).unambiguous

    def taps(self, k):
        if k not in self._taps:
            self._taps[k] = Taps(self, k)
        return self._taps[k]

    @property
    def t(self):
        return self.taps(self.k).t

    @property
    def ptm(self):
        return self.taps(self.k).ptm


class Taps:
    """Impulse response of Sync s at coarse offset k: M (|h|^2), dM, score, dscore, peak set, accepted taps."""

    def __init__(self, s, k):
        Z = np.where(CARRIER, np.roll(s.X, -k) * np.conj(R), 0.0)
        h = np.fft.ifft(Z)
        self.M = np.abs(h) ** 2
        dh = (math.sqrt(CARRIER.sum()) * s.E + C_FFT * LOG2N * U * math.sqrt((np.abs(Z) ** 2).sum())) / N
        self.dM = 2 * np.abs(h) * dh + dh * dh + 3 * U * self.M
        tot = self.M.sum()
        self.mean = tot / N
        self.dmean = (self.dM.sum() + gamma(N) * tot) / N + U * self.mean
        w = 1.0 - (1.0 - s.p) * np.abs(T_OF - s.expected) / NB_SYM
        dw = 5 * U
        self.score = self.M * w * w
        self.dscore = self.dM * w * w + self.M * (2 * np.abs(w) * dw + dw * dw) + 2 * U * self.score
        if not tot > 0:
            self.peak, self.peaks, self.t, self.ptm = 0, [0], 0, 0.0
            self.accepted, self.unambiguous = {0}, True
            self.ptm_of = {0: (0.0, 0.0)}
            return
        self.peak = int(np.argmax(self.score))
        self.peaks = [int(i) for i in indistinguishable(self.score, self.dscore)]
        self.accepted = set()
        self.ptm_of = {}
        nominal = None
        for pk in self.peaks:
            ptm = self.M[pk] / self.mean
            self.ptm_of[pk] = (ptm, ptm * (self.dM[pk] / self.M[pk] + self.dmean / self.mean + U))
            taps, nom = self._first_path(s, pk)
            self.accepted |= taps
            if pk == self.peak:
                nominal = nom
        self.t = signed_tap(nominal)
        self.ptm = self.ptm_of[self.peak][0]
        self.unambiguous = len(self.accepted) == 1 and len(self.peaks) == 1

    def _first_path(self, s, pk):
        """(accepted taps, the nominal tap) for score peak pk."""
        if not s.rel > 0:
            return {pk}, pk
        a, b = s.rel * self.M[pk], 16.0 * self.mean
        thr = max(a, b)
        dthr = max(s.rel * self.dM[pk] + 2 * U * a, 16.0 * self.dmean + U * b)
        d = np.arange(NB_CP, 0, -1)                              # earliest first
        n = (pk - d) % N
        m, dm = self.M[n], self.dM[n]
        sure = m - dm >= thr + dthr
        maybe = m + dm >= thr - dthr
        nominal = int(n[np.argmax(m >= thr)]) if (m >= thr).any() else pk
        acc = set()
        for i in range(len(d)):
            if maybe[i]:
                acc.add(int(n[i]))
            if sure[i]:
                break
        else:
            acc.add(pk)
        return acc, nominal


# ------------------------------------------------------------------------------------------------------ acceptance
def check_sync(s, k, t, ptm, cptm, label=""):
    """Hold one kernel result to Sync s; returns the largest error as a fraction of its budget (ratios)."""
    assert k in s.k_set, "%s: k %d not in %s (ref %d)" % (label, k, sorted(s.k_set), s.k)
    if len(s.k_set) == 1:
        assert k == s.k
    tp = s.taps(k)
    n = t % N
    assert n in tp.accepted, "%s: t %d not among %s (ref %d)" % (label, t, sorted(signed_tap(i) for i in tp.accepted), s.t)
    if tp.unambiguous and len(s.k_set) == 1:
        assert t == s.t, "%s: t %d != %d" % (label, t, s.t)
    worst = 0.0
    # ratios: within budget of the value at the kernel's k and at one of the indistinguishable peaks
    want_c, rel_c = s.cptm_of(k), s.cptm_rel(k)
    if want_c == 0.0:
        assert cptm == 0.0, "%s: coarse ratio %r of a zero correlation" % (label, cptm)
    else:
        e = abs(cptm - want_c) / (rel_c * want_c)
        assert e <= 1.0, "%s: coarse_peak_to_mean %r vs %r (%.2f budgets)" % (label, cptm, want_c, e)
        worst = max(worst, e)
    errs = [abs(ptm - v) / b if b > 0 else (0.0 if ptm == v else np.inf) for v, b in tp.ptm_of.values()]
    e = min(errs)
    assert e <= 1.0, "%s: peak_to_mean %r vs %r (%.2f budgets)" % (label, ptm, s.ptm, e)
    return max(worst, e)


def threshold_ok(value, budget, thr, got):
    """A >= threshold decision: exact unless value lies within budget of thr."""
    if abs(value - thr) <= budget:
        return True
    return bool(got) == bool(value >= thr)


# ------------------------------------------------------------------------------------------------------ null search
def block_l1(iq):
    x = np.asarray(iq).astype(np.complex128).reshape(-1)
    nb = x.size // 64
    v = np.abs(x[:nb * 64].real) + np.abs(x[:nb * 64].imag)
    return v.reshape(nb, 64).sum(axis=1)


def levels(l1, level_chunk):
    """Level per block: the capture's mean, or the local level (level_chunk > 0)."""
    nb = l1.size
    if level_chunk <= 0:
        return np.full(nb, l1.mean())
    nc = -(-nb // level_chunk)
    cm = np.array([l1[c * level_chunk:min(nb, (c + 1) * level_chunk)].mean() for c in range(nc)])
    lev = np.array([cm[max(0, c - 2):min(nc, c + 3)].mean() for c in range(nc)])
    return np.repeat(lev, level_chunk)[:nb]


def dip_machine(low, high, n_samples, min_blocks, max_out):
    """Candidates from per-block decisions low (l1 < ts) and high (l1 > te)."""
    out = []
    state, begin = 0, 0
    for b in range(low.size):
        if len(out) >= max_out:
            break
        if state == 0:
            if low[b]:
                state, begin = 1, b
        elif high[b]:
            ln = b - begin
            c = b * 64 - 48
            if min_blocks <= ln <= MAX_DIP_BLOCKS and c >= 0 and c + FRAME_LEN + 512 <= n_samples:
                out.append(c)
            state = 0
    return out


class NullSearch:
    """Candidates of one capture: .cands (the reference's), .alternatives (every list the in-band decisions allow),
    .n_in_band (block decisions within their band)."""

    MAX_FLIPS = 10

    def __init__(self, iq, thr_start=0.35, thr_end=0.75, min_blocks=30, level_chunk=256, max_out=64):
        x = np.asarray(iq).reshape(-1)
        n_samples = x.size
        self.l1 = block_l1(x)
        lev = levels(self.l1, level_chunk)
        ts = float(np.float32(thr_start)) * lev
        te = float(np.float32(thr_end)) * lev
        dl1 = gamma(127) * self.l1
        low, high = self.l1 < ts, self.l1 > te
        amb_lo = np.abs(self.l1 - ts) <= dl1 + 129 * U * ts
        amb_hi = np.abs(self.l1 - te) <= dl1 + 129 * U * te
        self.cands = dip_machine(low, high, n_samples, min_blocks, max_out)
        flips = [(b, 0) for b in np.flatnonzero(amb_lo)] + [(b, 1) for b in np.flatnonzero(amb_hi)]
        self.n_in_band = len(flips)
        assert len(flips) <= self.MAX_FLIPS, "capture ill-formed: %d block decisions in band" % len(flips)
        alts = set()
        for mask in itertools.product((False, True), repeat=len(flips)):
            lo, hi = low.copy(), high.copy()
            for (b, which), f in zip(flips, mask):
                if f:
                    (lo if which == 0 else hi)[b] ^= True
            alts.add(tuple(dip_machine(lo, hi, n_samples, min_blocks, max_out)))
        self.alternatives = alts
        self.unambiguous = len(alts) == 1


# ------------------------------------------------------------------------------------------------------ acquisition
class Acquired:
    """Reference for the acquired frame of candidate cand; .branches: one or two (fine, Sync) pairs (two where the
    cyclic-prefix angle lies within its band of +-pi)."""

    def __init__(self, iq, cand, max_coarse=200, min_peak_to_mean=30.0, margin=64, distance_prob=0.15,
                 first_path_rel=0.25):
        x = np.asarray(iq).astype(np.complex128).reshape(-1)
        self.n_samples = x.size
        self.cand = int(cand)
        self.margin = int(margin)
        self.min_ptm = float(np.float32(min_peak_to_mean))
        a = x[cand + CP_FIRST:cand + CP_LAST]
        b = x[cand + CP_FIRST + N:cand + CP_LAST + N]
        c = (np.conj(a) * b).sum()
        dc = 4 * U * (np.abs(a) * np.abs(b)).sum()
        self.theta = float(np.angle(c))
        self.dtheta = math.asin(min(1.0, dc / abs(c))) if abs(c) > 0 else math.pi
        w = x[cand:cand + NB_SYM]
        kw = dict(max_coarse=max_coarse, expected=0, distance_prob=distance_prob, first_path_rel=first_path_rel)
        thetas = [self.theta]
        if math.pi - abs(self.theta) <= self.dtheta:
            thetas.append(self.theta - math.copysign(2 * math.pi, self.theta))
        self.branches = []
        for th in thetas:
            fine = float(np.float32(-th / (2 * math.pi * N)))
            self.branches.append((fine, Sync(w, np.float32(fine), **kw)))
        self.fine, self.sync = self.branches[0]
        self.dfine = self.dtheta / (2 * math.pi * N) + 2 * U * abs(self.fine)      # (both sides round to float32)

    @property
    def unambiguous(self):
        return len(self.branches) == 1 and self.sync.unambiguous

    def start(self, sync=None):
        return self.cand + (sync or self.sync).t - self.margin


def check_acquired(ref, got, label=""):
    """got: one dabgpu_acquired_frame record.  Returns the largest error as a fraction of its budget."""
    fails = []
    for fine, s in ref.branches:
        try:
            return _check_branch(ref, fine, s, got, label)
        except AssertionError as e:
            fails.append(str(e))
    raise AssertionError(" / ".join(fails))


def _check_branch(ref, fine, s, got, label):
    k = int(got["coarse_carriers"])
    start = int(got["start"])
    t = start - ref.cand + ref.margin
    worst = check_sync(s, k, t, float(got["peak_to_mean"]), float(got["coarse_peak_to_mean"]), label)
    e = abs(float(got["fine_offset"]) - fine) / ref.dfine
    assert e <= 1.0, "%s: fine %r vs %r (%.2f budgets)" % (label, float(got["fine_offset"]), fine, e)
    worst = max(worst, e)
    want_f = fine - k / N
    df = ref.dfine + U * (abs(fine) + abs(k) / N)
    e = abs(float(got["freq_offset"]) - want_f) / df
    assert e <= 1.0, "%s: freq_offset %r vs %r" % (label, float(got["freq_offset"]), want_f)
    worst = max(worst, e)
    tp = s.taps(k)
    ptm_ok = any(threshold_ok(v, b, ref.min_ptm, int(got["flags"]) & 1) for v, b in tp.ptm_of.values())
    assert ptm_ok, "%s: lock bit %d, peak_to_mean %r vs threshold %r" % (label, int(got["flags"]) & 1, s.ptm, ref.min_ptm)
    inside = start >= 0 and start + FRAME_LEN <= ref.n_samples
    assert bool(int(got["flags"]) & 2) == inside, "%s: flags %d, start %d" % (label, int(got["flags"]), start)
    return max(worst, e)
