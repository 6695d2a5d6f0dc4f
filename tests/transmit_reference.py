"""The transmitter of include/dabgpu.h, "ETI(NI) to IQ", from the definition: integer numpy for the bits and the carrier
phases, float64 / complex128 for the samples.  Written without the library, oracle/ or modulator_reference (the
composition of dabgpu/synth.py), so that a misreading they share does not reach the judge.  It composes the pieces the
tests already own -- decoder_reference (mother code, puncturing vectors as the standard prints them, PRBS, profiles, time
interleaver), ofdm_reference (frequency interleaver), sync_reference (the phase reference symbol R by FFT bin),
tii_reference (carrier sets), eti_reference (the input frames) -- and adds the four steps that were missing:

  frame_bits   ETI contents -> the 230 400 bits of every transmission frame
  spectrum     bits -> the phase of every carrier of every symbol as an integer number of eighth turns
  modulate     bits -> samples (complex128)
  demap        samples -> the complex value of every FFT bin of every symbol (reads a modulator's output without a receiver)

A stream is a dict {id, start, bitrate, uep (bool), eep_type (0 = A, 1 = B), level (1..)} as in eti_reference.

Definitions.  Transmission frame f is made of ETI frames 4f .. 4f + 3.  FIC: the 96 bytes of ETI frame 4f + j are
scrambled, encoded and punctured to 2304 bits, four codewords = bits 0..9215.  MSC: the stream's bytes of ETI frame r give
coded[r] (scrambled, encoded, punctured, zero-padded to 64 * size bits); bit i of the sub-channel in CIF t is
coded[t - D(i mod 16)][i], zero before the start of the stream; the sub-channel lies at CIF bit 64 * start; CIF j of the
frame is bits 9216 + 55296 j ...  Block l - 1 (3072 bits) modulates symbol l = 1..75: carrier k_n of data index n turns by
(1 + 2 q) eighth turns, q = 0, 1, 2, 3 for (p_n, p_(n+1536)) = (0,0), (1,0), (1,1), (0,1), so that
e[l][n] = 2 prs(k_n) + l + 2 sum_{m <= l} q_m[n]  (mod 8)  and  z_l[k_n] = exp(j pi e / 4),  symbol 0 the phase reference.
A symbol is x[i] = gain / sqrt(1536) * sum_k z[k] exp(2 pi j k i / 2048), i = 0..2047, behind its last 504 samples.  The
null symbol is 2656 zeros, or the TII symbol of (main, sub): the 32 carriers of tii_reference.transmitter_carriers(sub,
main) with R's phase, the same sum, sample i of the 2656 being x[(i - 608) mod 2048].

Error budgets.  U = 2^-24, C_FFT = 7 per radix-2 stage and LOG2N = 11 are ofdm_reference's (Higham, theorem 24.2), and
like there a 2-norm bound of a transform's output is spread over its 2048 elements.  A correct float32 modulator that
starts from the exact points exp(j pi e / 4) -- `integers all the way', nothing accumulates over the frame -- does this:
- the points: 0 and +-1 are exact, 1 / sqrt 2 is one rounded constant: C_IN = 1 (a relative error of at most U on the
  spectrum's 2-norm);
- one 2048-point transform: C_FFT LOG2N U of the output's 2-norm.  The symbol has unit mean power, ||x||_2 =
  |gain| sqrt(2048), so the root mean square per sample is (C_FFT LOG2N + C_IN) U |gain| = 78 U |gain|;
- one final scaling by gain / sqrt(1536): the rounded constant, its product with the gain and the product with the
  sample, C_OUT = 3 roundings relative to the sample itself.
  SAMPLE budget   B[i] = (C_FFT LOG2N + C_IN) U |gain| + C_OUT U |x[i]|         (4.65e-6 + 1.8e-7 |x[i]| at unit gain)
- demap() is X[b] = sqrt(1536) / 2048 * sum_i x[504 + i] exp(-2 pi j b i / 2048) in float64 (its own rounding, 1e-15, is
  not budgeted), a carrier of the modulator is |gain| there.  ||dX||_2 = sqrt(1536 / 2048) ||dx||_2 and ||dx||_2 <=
  (C_FFT LOG2N + C_IN + C_OUT) U |gain| sqrt(2048); spread over the 2048 bins:
  CARRIER budget  E = sqrt(1536 / 2048) (C_FFT LOG2N + C_IN + C_OUT) U |gain|    (4.18e-6 |gain|)
  Neighbouring eighth-turn points are 2 sin(pi / 8) = 0.77 |gain| apart: the nearest point is never in doubt.
- The TII symbol is a direct sum of 32 unit terms, not a transform: gamma_31 times the sum of the terms' magnitudes (32)
  for the additions in any order, C_SINCOS = 4 U per component of a term (2 ulp of a value below 1, the argument -- an
  integer number of 2048ths of a turn -- is exact), C_OUT as above; both components, so sqrt 2:
  TII SAMPLE budget  B_tii = sqrt 2 (31 + C_SINCOS + C_OUT) 32 / sqrt(1536) U |gain|   (2.6e-6 |gain|), and per bin of
  demap_null() sqrt(1536 / 2048) of that.
The 1e-4 of the frame's peak that tests/test_modulator.py allows stays the ceiling: the peak of a frame is above 1 (unit
mean power), so it is above 1e-4, and B[i] <= 4.65e-6 + 1.8e-7 peak lies under it by a factor of twenty
(test_modulator_reference.py asserts it on every case it runs).

A refused ETI frame counts as 96 zero FIC bytes and zero stream bytes."""
import numpy as np

import decoder_reference as D
import eti_reference as E
import ofdm_reference as O
import sync_reference as S
import tii_reference as T

NB_FFT, NB_CP, NB_SYM, NB_SYMBOLS, NB_CARRIERS = O.NB_FFT, O.NB_CP, O.NB_SYM, O.NB_SYMBOLS, O.NB_CARRIERS
NB_NULL = 2656
NB_SYM_BITS = 2 * NB_CARRIERS
NB_FIC_BITS, NB_CIF_BITS = D.NB_FIC_BITS, D.NB_CIF_BITS
NB_FRAME_BITS = 75 * NB_SYM_BITS
NB_FRAME_SAMPLES = NB_NULL + NB_SYMBOLS * NB_SYM
assert NB_FRAME_BITS == NB_FIC_BITS + 4 * NB_CIF_BITS and NB_FRAME_SAMPLES == 196608
BAD_INPUT, MISALIGNED = 1, 2

U, C_FFT, LOG2N = O.U, O.C_FFT, O.LOG2N
C_IN, C_OUT, C_SINCOS = 1.0, 3.0, 4.0
SCALE = NB_FFT / np.sqrt(NB_CARRIERS)              # ifft(spec) * SCALE has unit mean power

_R = np.sqrt(0.5)
POINTS = np.array([1, _R + 1j * _R, 1j, -_R + 1j * _R, -1, -_R - 1j * _R, -1j, _R - 1j * _R], np.complex128)
PRS_QT = np.rint(np.angle(S.R[O.DATA_BINS]) / (np.pi / 2)).astype(np.int64) % 4     # quarter turns of R at data index n
assert np.abs(S.R[O.DATA_BINS] - 1j ** PRS_QT).max() == 0.0
UNUSED_BINS = np.setdiff1d(np.arange(NB_FFT), O.DATA_BINS)


def sample_budget(ref, gain=1.0):
    """B[i] for reference samples `ref` (any shape)."""
    return (C_FFT * LOG2N + C_IN) * U * abs(gain) + C_OUT * U * np.abs(ref)


def carrier_budget(gain=1.0):
    return np.sqrt(NB_CARRIERS / NB_FFT) * (C_FFT * LOG2N + C_IN + C_OUT) * U * abs(gain)


def tii_sample_budget(gain=1.0):
    return np.sqrt(2.0) * (31 + C_SINCOS + C_OUT) * 32 / np.sqrt(NB_CARRIERS) * U * abs(gain)


def tii_carrier_budget(gain=1.0):
    return np.sqrt(NB_CARRIERS / NB_FFT) * tii_sample_budget(gain)


# ------------------------------------------------------------------------------------------------ profiles, ETI frames
_UEP = None


def uep_rows():
    """The 64 UEP profiles in table order (decoder_reference.uep_profile: each row behind its two identities)."""
    global _UEP
    if _UEP is None:
        _UEP = [D.uep_profile(i) for i in range(64)]
    return _UEP


def uep_index(bitrate, level):
    for i, p in enumerate(uep_rows()):
        if (p.bitrate, p.level) == (bitrate, level):
            return i
    raise ValueError("no UEP row for %d kbit/s at level %d" % (bitrate, level))


def profile_of(st):
    if st["uep"]:
        return uep_rows()[uep_index(st["bitrate"], st["level"])]
    return D.eep_profile(st["eep_type"], st["level"], st["bitrate"])


def build_eti(streams, fibs, data, count0=0):
    """ETI frames [n_cif][6144] (uint8) from fibs [n_cif][3][32] and data {id: [n_cif][bitrate * 3]} with the reference
    writer; frame t carries CIF count count0 + t."""
    n_cif = len(fibs)
    out = np.zeros((n_cif, E.FRAME_BYTES), np.uint8)
    for t in range(n_cif):
        fr = E.write_frame(streams, (count0 + t) % 5000, np.asarray(fibs[t], np.uint8).tobytes(),
                           {i: np.asarray(d[t], np.uint8).tobytes() for i, d in data.items()}, 0xFF)
        out[t] = np.frombuffer(fr, np.uint8)
    return out


def status(n_cif, refused=(), count0=0):
    """[(flags, refused mask)] per transmission frame."""
    out = []
    for f in range(n_cif // 4):
        m = sum(1 << j for j in range(4) if 4 * f + j in set(refused))
        out.append(((BAD_INPUT if m else 0) | (MISALIGNED if (count0 + 4 * f) % 4 else 0), m))
    return out


# ------------------------------------------------------------------------------------------------ bits
_PRBS = D.prbs(1152 * 8)


def _scrambled(byte_rows):
    bits = np.unpackbits(np.asarray(byte_rows, np.uint8), axis=1)
    pr = _PRBS if bits.shape[1] <= _PRBS.size else D.prbs(bits.shape[1])
    return bits ^ pr[None, :bits.shape[1]]


def coded_records(profile, byte_rows):
    """byte_rows [n][nbytes] -> [n][kept + padding]: dispersal, mother code, puncturing, zero padding."""
    mother = D.conv_encode(_scrambled(byte_rows))
    assert mother.shape[1] == profile.mask.size
    out = np.zeros((mother.shape[0], profile.kept + profile.padding), np.uint8)
    out[:, :profile.kept] = mother[:, profile.mask.astype(bool)]
    return out


def frame_bits(streams, fibs, data, refused=(), history=None, return_history=False):
    """The 230 400 bits of every transmission frame of ONE stream -> uint8 [n_cif / 4][230400].  fibs [n_cif][3][32], data
    {id: [n_cif][bitrate * 3]}; refused: the ETI frames of this call that are not taken (zero bytes).  history: None (the
    stream starts with this call) or {id: [15][64 * size]}, the coded records of the 15 ETI frames before this call;
    return_history: also return that dict for the next call."""
    fibs = np.array(fibs, np.uint8).reshape(-1, 96)
    n_cif = fibs.shape[0]
    assert n_cif % 4 == 0
    bad = sorted(set(refused))
    fibs[bad] = 0
    fic = coded_records(D.fic_profile(), fibs)                                     # [n_cif][2304]
    cifs = np.zeros((n_cif, NB_CIF_BITS), np.uint8)
    hist = {}
    for st in streams:
        p = profile_of(st)
        assert p.kept + p.padding == 64 * p.size_cu and 0 <= st["start"] and st["start"] + p.size_cu <= 864
        d = np.array(data[st["id"]], np.uint8).reshape(n_cif, st["bitrate"] * 3)
        d[bad] = 0
        old = np.zeros((15, 64 * p.size_cu), np.uint8) if history is None else np.asarray(history[st["id"]], np.uint8)
        rows = np.concatenate([old, coded_records(p, d)])                          # row 15 + r = coded[r]
        a = 64 * st["start"]
        assert not cifs[:, a:a + 64 * p.size_cu].any()
        cifs[:, a:a + 64 * p.size_cu] = D.time_interleave(rows)[15:15 + n_cif]     # bit i of row r goes out D(i mod 16) later
        hist[st["id"]] = rows[-15:]
    bits = np.concatenate([fic.reshape(n_cif // 4, NB_FIC_BITS), cifs.reshape(n_cif // 4, 4 * NB_CIF_BITS)], axis=1)
    return (bits, hist) if return_history else bits


def locate(streams, f, b):
    """Where bit b of transmission frame f comes from, in words."""
    sym = "frame %d, data symbol %d, " % (f, b // NB_SYM_BITS + 1)
    if b < NB_FIC_BITS:
        return sym + "FIC codeword %d bit %d" % divmod(b, 2304)
    j, i = divmod(b - NB_FIC_BITS, NB_CIF_BITS)
    for st in streams:
        a, n = 64 * st["start"], 64 * profile_of(st).size_cu
        if a <= i < a + n:
            return sym + "CIF %d (ETI frame %d), sub-channel id %d at CU %d, bit %d of %d" % (j, 4 * f + j, st["id"], st["start"], i - a, n)
    return sym + "CIF %d (ETI frame %d), unallocated bit %d (CU %d)" % (j, 4 * f + j, i, i // 64)


# ------------------------------------------------------------------------------------------------ carriers and samples
def spectrum(bits):
    """bits [n][230400] -> e [n][76][1536] (int64): carrier k_n = ofdm_reference.CARRIERS[n] of symbol l is
    exp(j pi e[l][n] / 4); symbol 0 is the phase reference symbol."""
    b = np.asarray(bits, np.uint8).reshape(-1, 75, 2, NB_CARRIERS).astype(np.int64)
    p0, p1 = b[:, :, 0], b[:, :, 1]
    q = (p0 ^ p1) + 2 * p1                                                         # (0,0) (1,0) (1,1) (0,1) -> 0 1 2 3
    e = np.zeros((b.shape[0], NB_SYMBOLS, NB_CARRIERS), np.int64)
    e[:, 0] = 2 * PRS_QT
    e[:, 1:] = 2 * PRS_QT + np.arange(1, NB_SYMBOLS)[None, :, None] + 2 * np.cumsum(q, axis=1)
    return e % 8


def bits_of(e):
    """The differential decision: exponents [n][76][1536] -> (bits [n][230400], ok [n][75][1536]: the step between two
    symbols is an odd number of eighth turns, as every dibit's is)."""
    step = (e[:, 1:] - e[:, :-1]) % 8
    q = (step - 1) // 2 % 4
    p1 = q >> 1
    p0 = (q & 1) ^ p1
    return np.stack([p0, p1], axis=2).reshape(e.shape[0], -1).astype(np.uint8), step % 2 == 1


def tii_symbol(main, sub):
    """The 2656 samples of the TII null symbol of transmitter (main, sub) at unit gain, complex128."""
    spec = np.zeros(NB_FFT, np.complex128)
    for k in T.transmitter_carriers(sub, main):
        spec[k % NB_FFT] = S.R[k % NB_FFT]
    t = np.fft.ifft(spec) * SCALE
    return t[(np.arange(NB_NULL) - (NB_NULL - NB_FFT)) % NB_FFT]


def modulate(bits, tii=None, gain=1.0):
    """bits [n][230400] -> complex128 [n][196608]; tii = (main, sub) or None (a null symbol of zeros)."""
    e = spectrum(bits)
    n = e.shape[0]
    spec = np.zeros((n, NB_SYMBOLS, NB_FFT), np.complex128)
    spec[:, :, O.DATA_BINS] = POINTS[e]
    t = np.fft.ifft(spec, axis=-1) * (SCALE * gain)
    out = np.zeros((n, NB_FRAME_SAMPLES), np.complex128)
    if tii is not None:
        out[:, :NB_NULL] = tii_symbol(*tii)[None, :] * gain
    sym = out[:, NB_NULL:].reshape(n, NB_SYMBOLS, NB_SYM)
    sym[:, :, :NB_CP] = t[:, :, -NB_CP:]
    sym[:, :, NB_CP:] = t
    return out


def demap(iq):
    """iq [n][>= 196608] -> X [n][76][2048] complex128 by FFT bin: the float64 FFT of samples 504..2551 of every symbol,
    scaled so that a carrier of a unit-gain modulator has magnitude 1."""
    x = np.asarray(iq)
    x = x.reshape(-1, x.shape[-1])[:, NB_NULL:NB_FRAME_SAMPLES].astype(np.complex128).reshape(-1, NB_SYMBOLS, NB_SYM)
    return np.fft.fft(x[:, :, NB_CP:], axis=-1) / SCALE


def demap_null(iq):
    """iq [n][>= 2656] -> [n][2048]: the same of the last 2048 samples of every null symbol."""
    x = np.asarray(iq)
    x = x.reshape(-1, x.shape[-1])[:, NB_NULL - NB_FFT:NB_NULL].astype(np.complex128)
    return np.fft.fft(x, axis=-1) / SCALE


def nearest_points(X):
    """X [...][2048] (demap) -> (e [...][1536] nearest eighth-turn exponent per data index, |X| on the unused bins)."""
    Xd = X[..., O.DATA_BINS]
    e = np.rint(np.angle(Xd) / (np.pi / 4)).astype(np.int64) % 8
    return e, np.abs(X[..., UNUSED_BINS])
