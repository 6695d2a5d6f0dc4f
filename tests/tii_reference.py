"""Transmitter identification (EN 300 401 section 14.8, Mode I) restated from the definition in numpy, for the tests of
dabgpu_tii_*: the carrier sets, the pattern table (generated here, not copied from the library), the per-frame records
(window -> frequency correction -> float64 FFT -> cells / floor) and the decode rule.

The two conventions restated from memory -- which bit of a pattern is position b = 0, and the four carrier bases -- are
kept here once, as they are kept once in the library (csrc/kernels.hpp).  What the tests pin is that the two agree and that
the bases partition the 1536 carriers, not the standard's numbering.

The frequency correction is the one the kernels apply: the correction f is taken as the float32 the device holds and
quantised to the 32-bit phase step dphi = llrint(f 2^32) mod 2^32 (ties to even); sample n of the WINDOW (n = 0 at its
first sample) is multiplied by exp(2 pi i frac(n dphi / 2^32)), the phase formed in exact integer arithmetic
(ofdm_reference.dphi_of / nco).  dphi = 0 leaves the samples as they are.

Error budgets.  U = 2^-24; every budget is a forward-error bound of a correct float32 implementation of the same
operation, built as ofdm_reference.py builds its own (Higham: sums section 3.1, FFT theorem 24.2; C_FFT = 7 per radix-2
stage).
- C_NCO_DIRECT = 8 is the constant of the direct nco(n, dphi) these kernels call, with no running rotation: per sample
  the phase float(int32 n dphi) carries half an ulp of a 24-bit mantissa (2^-26 of a turn: 2 pi 2^-26 = 1.6 U in the
  phasor), sincospif 2 ulp per component (2 sqrt 2 U = 2.9 U), and the complex product two roundings per component
  (3 U): 7.5 U, rounded up.  It is a sixteenth of ofdm_reference.C_NCO (128), which pays for 15 rotations of a running
  phasor, and it is 0 where dphi == 0 (the kernels skip the product).
- Spectrum: E_X = (C_FFT 11 + C_nco) U ||y||_2 per bin, y the 2048 corrected samples: the 2-norm bound of the whole
  transform spread over its bins (Parseval), as ofdm_reference's E_l.
- A power |X_k|^2 moves by at most 2 |X_k| E_X + E_X^2, and its own arithmetic (two products, one sum) by
  gamma_2 (|X_k| + E_X)^2.
- Cell: 8 powers summed in order: sum (2 |X_k| E_X + E_X^2) + C_CELL U sum (|X_k| + E_X)^2, C_CELL = 2 + 8 (gamma_2
  of a power, gamma_7 of the sum, rounded up).
- Floor: the mean of 304 powers through a fixed tree: two powers added per lane (1), six levels inside a wave (6),
  the four waves in order (3), the division by 304 (1), on top of a power's gamma_2: C_FLOOR = 13, so
  (sum (2 |X_k| E_X + E_X^2) + C_FLOOR U sum (|X_k| + E_X)^2) / 304.
The accumulators carry no budget: a call's sum is bit for bit the sequential float32 frame-order sum of its records
added to what the accumulator held, the frame count added as an integer."""
import math

import numpy as np

from ofdm_reference import C_FFT, C_NCO, LOG2N, U, dphi_of, nco

C_NCO_DIRECT, C_CELL, C_FLOOR = 8.0, 10.0, 13.0
assert C_NCO_DIRECT <= C_NCO

NB_FFT = 2048
COMBS, POSITIONS, PATTERNS = 24, 8, 70
BASES = (-768, -384, 1, 385)
WIN_BEGIN, WIN_END = 2352, 304          # window [-2352, -304) relative to the PRS prefix
FLOOR_LO, FLOOR_HI = 776, 927


def patterns():
    """The 70 four-of-eight subsets as 8-bit values, ascending (pattern p = patterns()[p])."""
    return [v for v in range(256) if bin(v).count("1") == 4]


def positions(p):
    """Positions b switched on by pattern p (bit 7 - b of its value)."""
    v = patterns()[p]
    return [b for b in range(POSITIONS) if v >> (7 - b) & 1]


def cell_carriers(c, b):
    """The 8 carriers k of cell (c, b): per base, the pair B + 2c + 48b and the next carrier."""
    return [k for B in BASES for k in (B + 2 * c + 48 * b, B + 2 * c + 48 * b + 1)]


def transmitter_carriers(c, p):
    """The 32 carriers of transmitter (c, p)."""
    return sorted(k for b in positions(p) for k in cell_carriers(c, b))


def noise_bins():
    k = np.arange(FLOOR_LO, FLOOR_HI + 1)
    return np.concatenate([k, NB_FFT - k])


CELL_BINS = np.array([[[k % NB_FFT for k in cell_carriers(c, b)] for b in range(POSITIONS)] for c in range(COMBS)])


def spectrum(window, freq_offset=0.0):
    """(X [2048] complex128, E_X): the corrected window's transform and its per-bin budget."""
    x = np.asarray(window, np.complex128).reshape(NB_FFT)
    dphi = dphi_of(freq_offset)
    y = x * nco(NB_FFT, dphi) if dphi else x
    e = (C_FFT * LOG2N + (C_NCO_DIRECT if dphi else 0.0)) * U * math.sqrt(float((np.abs(y) ** 2).sum()))
    return np.fft.fft(y), e


def power_terms(X, e):
    """Per bin: (|X|^2, what the spectral budget moves it by, the bound its own rounding scales with)."""
    m = np.abs(X)
    return m ** 2, 2.0 * m * e + e * e, (m + e) ** 2


def record(window, freq_offset=0.0, budgets=False):
    """One frame: window = the 2048 samples [-2352, -304) before its PRS prefix -> (cells [24][8], floor), float64, and
    with budgets=True also (cell budget [24][8], floor budget).  The correction starts at the window's first sample."""
    X, e = spectrum(window, freq_offset)
    P, dP, R = power_terms(X, e)
    cells = P[CELL_BINS].sum(axis=2)
    nb = noise_bins()
    floor = P[nb].mean()
    if not budgets:
        return cells, floor
    cell_b = dP[CELL_BINS].sum(axis=2) + C_CELL * U * R[CELL_BINS].sum(axis=2)
    floor_b = (dP[nb].sum() + C_FLOOR * U * R[nb].sum()) / nb.size
    return cells, floor, cell_b, floor_b


def records(iq, prs_starts, freq_offsets=None, budgets=False):
    """Records of the frames whose PRS prefixes start at prs_starts in the 1-D array iq -> (cells [n][24][8], floor [n]),
    with budgets=True also (cell budgets [n][24][8], floor budgets [n])."""
    out = []
    for i, s in enumerate(prs_starts):
        s = int(s)
        out.append(record(iq[s - WIN_BEGIN:s - WIN_END], 0.0 if freq_offsets is None else freq_offsets[i], budgets))
    return tuple(np.array(a) for a in zip(*out))


def decode(cells, floor, frames=1, min_level_db=3.0):
    """The decode rule on accumulated sums -> [(main_id, sub_id, level_db (float32), ambiguous)], strongest first, ties in
    (sub_id, main_id) order.  min_level_db is taken as the float32 the C struct holds."""
    if frames == 0 or not floor > 0.0:
        return []
    thr = math.pow(10.0, float(np.float32(min_level_db)) / 10.0)
    noise = 8.0 * float(np.float32(floor))
    out = []
    for c in range(COMBS):
        level = [float(np.float32(cells[c][b])) / noise - 1.0 for b in range(POSITIONS)]
        on = [lv >= thr for lv in level]
        for p in range(PATTERNS):
            bs = positions(p)
            if all(on[b] for b in bs):
                s = 0.0
                for b in bs:
                    s += level[b]
                out.append((p, c, float(np.float32(10.0 * math.log10(s / 4.0))), sum(on) > 4))
    return sorted(out, key=lambda e: -e[2])       # (stable: ties keep the (c, p) order)
