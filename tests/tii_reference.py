"""Transmitter identification (EN 300 401 section 14.8, Mode I) restated from the definition in numpy, for the tests of
dabgpu_tii_*: the carrier sets, the pattern table (generated here, not copied from the library), the per-frame records
(window -> frequency correction -> float64 FFT -> cells / floor) and the decode rule.

The two conventions restated from memory -- which bit of a pattern is position b = 0, and the four carrier bases -- are
kept here once, as they are kept once in the library (csrc/kernels.hpp).  What the tests pin is that the two agree and that
the bases partition the 1536 carriers, not the standard's numbering."""
import math

import numpy as np

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


def record(window, freq_offset=0.0):
    """One frame: window = the 2048 samples [-2352, -304) before its PRS prefix -> (cells [24][8], floor), float64.  The
    correction exp(2 pi i f n) starts at the window's first sample (the phase does not reach a power)."""
    x = np.asarray(window, np.complex128)
    if freq_offset:
        x = x * np.exp(2j * np.pi * float(freq_offset) * np.arange(NB_FFT))
    P = np.abs(np.fft.fft(x)) ** 2
    cells = np.zeros((COMBS, POSITIONS))
    for c in range(COMBS):
        for b in range(POSITIONS):
            cells[c, b] = sum(P[k % NB_FFT] for k in cell_carriers(c, b))
    return cells, P[noise_bins()].mean()


def records(iq, prs_starts, freq_offsets=None):
    """Records of the frames whose PRS prefixes start at prs_starts in the 1-D array iq -> (cells [n][24][8], floor [n])."""
    out_c, out_f = [], []
    for i, s in enumerate(prs_starts):
        s = int(s)
        c, f = record(iq[s - WIN_BEGIN:s - WIN_END], 0.0 if freq_offsets is None else freq_offsets[i])
        out_c.append(c)
        out_f.append(f)
    return np.array(out_c), np.array(out_f)


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
