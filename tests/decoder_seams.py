"""The inputs of tests/test_decoder_seams.py: sub-channels and plain codewords on either side of every kernel-selection
seam of the channel decoder, by the recipe of tests/decoder_profiles.py, and the exact reference's answers.  Imports numpy
and decoder_reference alone: nothing here comes from the library, the oracle or the tool that prints the seams.

A sub-channel's key is (EEP option, level, bit rate, salt); the salt tells copies of one profile apart that carry
different data.  Codewords: c [16][kept] int8 per key -- 0..3 signal at amplitude 60 with Gaussian noise at 8 dB, 4..9
uniform in -127..127, 10..15 on the 16-level grid 16 k + 8 (many exact ties): the 12 noise codewords are what shows a
single lost or misplaced soft bit.  The sub-channel's CIFs are cyclic with period 16 as in decoder_profiles: the logical
frame that is complete with CIF t is c[t mod 16], four frames are one period, history_in is the 15 CIFs before them
(rows 1..15 of the period: random and never NULL), history_out after any whole number of periods is the same rows, and
codeword t of a longer run is c[t mod 16].  Every capacity unit no entry uses holds uniform noise; the FIC of every
stream is the same four frames of noise, so that one reference decodes it."""
import functools

import numpy as np

import decoder_reference as R

N_CW = 16
NB_FRAME_BITS = 230400
SIGNAL, NOISE = (0, 1, 2, 3), tuple(range(4, 16))
SMALL = (0, 3, 64)                                       # the second, small sub-channel of a pair: 48 CU behind the first


@functools.lru_cache(maxsize=None)
def profile(key):
    return R.eep_profile(key[0], key[1], key[2])


def name(key):
    return "eep%d%s-%d#%d" % (key[1], "AB"[key[0]], key[2], key[3])


# ------------------------------------------------------------------------------------------------ codewords and periods
def _mix(rng, code_pm1, n_signal):
    """[n][kept] int64: n_signal rows of signal at 8 dB, the rest half uniform noise, half the 16-level grid."""
    n, kept = code_pm1.shape[0], code_pm1.shape[1]
    c = np.zeros((n, kept), np.int64)
    sigma = 60 / 10.0 ** (8.0 / 20.0)
    c[:n_signal] = np.clip(np.rint(code_pm1[:n_signal] * 60 + rng.normal(0.0, sigma, (n_signal, kept))), -127, 127)
    half = n_signal + (n - n_signal + 1) // 2
    c[n_signal:half] = rng.integers(-127, 128, (half - n_signal, kept))
    c[half:] = rng.integers(-8, 8, (n - half, kept)) * 16 + 8
    return c


@functools.lru_cache(maxsize=None)
def codewords(key):
    p = profile(key)
    rng = np.random.default_rng(list(key) + [0x5EA])
    msgs = rng.integers(0, 2, (N_CW, p.nsteps - 6), dtype=np.uint8)
    code = (R.conv_encode(msgs).astype(np.int64) * 2 - 1)[:, np.flatnonzero(p.mask)]
    c = _mix(rng, code, len(SIGNAL)).astype(np.int8)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def period(key):
    """The sub-channel's 16 CIFs int8 [16][64 size_cu]: CIF q of the cyclic transmission is row q mod 16."""
    p = profile(key)
    assert p.kept == 64 * p.size_cu                      # (EEP: no padding)
    sent = codewords(key)[(np.arange(48) + 15) % 16]     # the frame that STARTS with CIF r is complete with CIF r + 15
    cifs = R.time_interleave(sent)[16:32].copy()
    cifs.setflags(write=False)
    return cifs


def history(key):
    """history_in of the period's first CIF, and history_out after every whole period."""
    return period(key)[1:]


def cifs_of(key, n_cifs):
    """The first n_cifs CIFs of the cyclic transmission, and history_out behind them."""
    rows = period(key)[np.arange(n_cifs) % 16]
    return rows, np.concatenate([history(key), rows])[-15:]


@functools.lru_cache(maxsize=None)
def fic_noise():
    soft = np.random.default_rng(0xF1C5).integers(-127, 128, (4, R.NB_FIC_BITS), dtype=np.int8)
    soft.setflags(write=False)
    return soft


@functools.lru_cache(maxsize=None)
def fic_ref():
    return R.fic_reference(fic_noise())


@functools.lru_cache(maxsize=None)
def stream_frames(entries):
    """entries: tuple of (key, start CU) -> four whole frames int8 [4][230400]."""
    rng = np.random.default_rng([0x57EA] + [v for k, s in entries for v in list(k) + [s]])
    soft = rng.integers(-127, 128, (4, NB_FRAME_BITS), dtype=np.int8)
    soft[:, :R.NB_FIC_BITS] = fic_noise()
    cifs = soft[:, R.NB_FIC_BITS:].reshape(16, R.NB_CIF_BITS)
    at = 0
    for k, start in entries:
        assert start >= at and start + profile(k).size_cu <= 864, entries
        at = start + profile(k).size_cu
        cifs[:, 64 * start:64 * at] = period(k)
    soft[:, R.NB_FIC_BITS:] = cifs.reshape(4, 4 * R.NB_CIF_BITS)
    soft.setflags(write=False)
    return soft


def pair(key):
    """The stream of the per-length tests: the sub-channel at CU 3 (an odd unit, noise in front), a 64 kbit/s one with
    the same salt directly behind it, noise behind that."""
    return ((key, 3), (SMALL + (key[3] + 100 * key[0] + key[2],), 3 + profile(key).size_cu))


# ------------------------------------------------------------------------------------------------ the sub-channels
SEAM_RATES = (200, 208, 408, 416, 680, 688, 792, 800)     # both sides of the four seams of legal lengths (EEP 3-A)
LANE_RATES = (504, 520)                                   # wave kernels only: n_lanes 63 | 64, last segment whole | partial
MAIN = tuple((0, 3, b, 0) for b in SEAM_RATES) + ((1, 2, 416, 0), (1, 4, 800, 0))
WAVE_ONLY = tuple((0, 3, b, 0) for b in LANE_RATES)
TABLE = (((0, 3, 792, 0),), ((0, 3, 800, 0),), ((0, 3, 64, 7),))       # decode_ensembles_dev: three streams, each at CU 0
MANY = ((0, 3, 800, 0),) + tuple((0, 3, 8, j) for j in range(16))       # 600 + 16 x 6 CU
#: history rings on either side of the ride rule: (streams, key without salt); stream s carries salt s
RINGS = ((3, (0, 3, 480)), (4, (1, 2, 416)), (73, (1, 4, 32)), (3, (0, 3, 488)))
ONE_ROUND = (0, 3, 64, 9)                                 # the FIC with ONE sub-channel


def many_stream(n_small):
    at, out = 0, []
    for k in MANY[:1 + n_small]:
        out.append((k, at))
        at += profile(k).size_cu
    return tuple(out)


def ring_stream(key, s):
    """Stream s of a ring case: the sub-channel whose ring the case is about, and an 8 kbit/s one (6 CU) behind it, so that
    the first is the largest ring of the list, which is the one the ride rule looks at."""
    k = key + (s,)
    return ((k, 3), ((0, 3, 8, 50 + s % 3), 3 + profile(k).size_cu))


def ring_bytes(n_streams, key):
    """The size the launcher compares: the largest ring of the list, n_streams x 15 CIFs x the sub-channel's bits."""
    return max(n_streams * 15 * 64 * profile(k).size_cu for s in range(n_streams) for k, _ in ring_stream(key, s))


def all_keys():
    keys = set()
    for k in MAIN + WAVE_ONLY:
        keys |= {e[0] for e in pair(k)}
    keys |= {lst[0] for lst in TABLE} | set(MANY) | {ONE_ROUND}
    for n, key in RINGS:
        for s in range(n):
            keys |= {e[0] for e in ring_stream(key, s)}
    return sorted(keys)


@functools.lru_cache(maxsize=None)
def length_ref(nsteps):
    """One viterbi call for every key of this length, their codewords stacked."""
    keys = [k for k in all_keys() if profile(k).nsteps == nsteps]
    mother = np.concatenate([R.depuncture(codewords(k), profile(k).mask) for k in keys])
    d = R.viterbi(mother, stats=False)
    d.bits()
    return keys, mother, d


def ref(key):
    """-> mother int64 [16][4 nsteps], Decoded of the 16 codewords."""
    keys, mother, d = length_ref(profile(key).nsteps)
    i = keys.index(key)
    return mother[N_CW * i:N_CW * (i + 1)], d.lanes(np.arange(N_CW * i, N_CW * (i + 1)))


# ------------------------------------------------------------------------------------------------ plain codewords
PLAIN_N = 9
PLAIN_MASKS = ("pi1", "pi24", "full")


def plain_mask(nsteps, kind):
    return np.ones(4 * nsteps, np.uint8) if kind == "full" else R.plain_mask(nsteps, 1 if kind == "pi1" else 24)


@functools.lru_cache(maxsize=None)
def plain_case(nsteps, kind):
    """-> punctured soft bits int8 [9][kept]: 2 signal at 8 dB, 4 uniform, 3 on the grid."""
    mask = plain_mask(nsteps, kind)
    rng = np.random.default_rng([nsteps, PLAIN_MASKS.index(kind), 0x91A])
    msgs = rng.integers(0, 2, (PLAIN_N, nsteps - 6), dtype=np.uint8)
    code = (R.conv_encode(msgs).astype(np.int64) * 2 - 1)[:, np.flatnonzero(mask)]
    c = _mix(rng, code, 2).astype(np.int8)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def plain_ref(nsteps):
    """-> {kind: (mother [9][4 nsteps], Decoded)}, the three masks' codewords decoded in one call."""
    mother = np.concatenate([R.depuncture(plain_case(nsteps, k), plain_mask(nsteps, k)) for k in PLAIN_MASKS])
    d = R.viterbi(mother, stats=False)
    d.bits()
    return {k: (mother[PLAIN_N * i:PLAIN_N * (i + 1)], d.lanes(np.arange(PLAIN_N * i, PLAIN_N * (i + 1)))) for i, k in enumerate(PLAIN_MASKS)}
