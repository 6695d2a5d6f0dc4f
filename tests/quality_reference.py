"""Reception quality (include/dabgpu.h, "Reception quality") restated from its definition in numpy, for the tests of
dabgpu_mer_dev and dabgpu_channel_ber_dev.  Imports numpy and decoder_reference alone -- not the library, dabgpu/synth.py
or oracle/ -- and takes from decoder_reference the encoder, the energy dispersal sequence, the time de-interleaver and
the puncturing profiles, each of which that module states from EN 300 401 and its own tests pin.

MER.  A frame's soft bits are 75 data symbols of 3072 bytes; carrier n of a symbol is the pair (byte n, byte 1536 + n).
With a = |re|, b = |im| as integers (|-128| = 128): signal = sum (a + b)^2, error = sum (a - b)^2, carriers = the
number of pairs that are not (0, 0), over the symbols asked for.  Any int8 bytes are a valid input: nothing here
assumes they came out of the quantiser.

Channel BER.  A pure function of the soft bytes, the carried history, the sub-channel descriptor and the GIVEN decoded
bytes -- whether a decoder produced them is no concern of the count.  Per codeword: the decoded bytes (MSB first) are
scrambled again with the energy dispersal sequence, encoded with the mother code (six zero tail bits), punctured by the
profile's mask, and every kept bit is compared with the sign of the soft byte the time de-interleaver assigns to it
(positive = 1); a soft byte of 0 is no decision and is not counted.  The FIC is not interleaved: codeword g of a frame
is bytes 2304 g .. 2304 g + 2303, 3 FIBs.  MSC codeword t of a stream (its CIF index, 4 per frame) reads punctured bit
i from CIF t - 15 + bitrev4(i mod 16) of the same stream; CIFs before the stream's first come from the history
[15][64 size_cu] (row r = CIF r - 15), or are erased when there is none.  A UEP sub-channel's padding bits lie behind
the kept bits and are not read.

Both results are integers: everything is exact."""
import numpy as np

import decoder_reference as D

NB_CARRIERS, NB_SYM_BITS, NB_DATA_SYMBOLS = 1536, 3072, 75
NB_FIC_BITS, NB_CIF_BITS, NB_FRAME_BITS = D.NB_FIC_BITS, D.NB_CIF_BITS, 230400
NB_FIC_GROUP_BITS = 2304


def mer(soft, first_symbol=0, n_symbols=NB_DATA_SYMBOLS):
    """soft [n_frames][>= 230400] int8 -> (signal [n], error [n], carriers [n]) as exact int64 arrays, over data
    symbols [first_symbol, first_symbol + n_symbols)."""
    soft = np.atleast_2d(np.asarray(soft, np.int8))
    s = soft[:, :NB_FRAME_BITS].reshape(soft.shape[0], NB_DATA_SYMBOLS, NB_SYM_BITS)
    s = s[:, first_symbol:first_symbol + n_symbols].astype(np.int64)
    a, b = np.abs(s[..., :NB_CARRIERS]), np.abs(s[..., NB_CARRIERS:])
    return (((a + b) ** 2).sum(axis=(1, 2)), ((a - b) ** 2).sum(axis=(1, 2)), ((a != 0) | (b != 0)).sum(axis=(1, 2)))


_PRBS = {}


def dispersal(n):
    if n not in _PRBS:
        _PRBS[n] = D.prbs(n)
    return _PRBS[n]


def coded_bits(decoded_bytes, profile):
    """The kept (transmitted) coded bits [profile.kept] of one codeword's decoded bytes [profile.nbytes]."""
    bits = np.unpackbits(np.asarray(decoded_bytes, np.uint8).reshape(-1))
    assert bits.size == profile.nsteps - 6
    mother = D.conv_encode(bits ^ dispersal(bits.size))[0]
    return mother[profile.mask.astype(bool)]


def count(soft, coded):
    """(errors, bits) of soft bytes [n] against coded bits [n]."""
    soft = np.asarray(soft).astype(np.int64)
    decided = soft != 0
    return int((decided & ((soft > 0) != (np.asarray(coded) != 0))).sum()), int(decided.sum())


def fic_ber(soft, fib):
    """soft [n_frames][>= 9216] int8, fib [n_frames][12][32] uint8 (any bytes) -> (errors, bits), each [n_frames][4]."""
    soft = np.atleast_2d(np.asarray(soft, np.int8))
    fib = np.asarray(fib, np.uint8).reshape(soft.shape[0], 4, 96)
    p = D.fic_profile()
    out = np.zeros((2, soft.shape[0], 4), np.int64)
    for f in range(soft.shape[0]):
        for g in range(4):
            out[:, f, g] = count(soft[f, NB_FIC_GROUP_BITS * g:NB_FIC_GROUP_BITS * (g + 1)], coded_bits(fib[f, g], p))
    return out[0], out[1]


def msc_ber(soft, start_cu, profile, decoded, history=None):
    """One stream's sub-channel: soft [n_frames][>= 230400] int8, the sub-channel at capacity unit start_cu with
    decoder_reference profile `profile`, decoded [4 n_frames][profile.nbytes] uint8 (any bytes), history [15][64 size_cu]
    int8 or None -> (errors, bits), each [4 n_frames]."""
    soft = np.atleast_2d(np.asarray(soft, np.int8))
    nbits = 64 * profile.size_cu
    assert 0 <= start_cu and start_cu + profile.size_cu <= 864 and profile.kept + profile.padding == nbits
    cifs = soft[:, NB_FIC_BITS:NB_FRAME_BITS].reshape(-1, NB_CIF_BITS)[:, 64 * start_cu:64 * start_cu + nbits]
    logical, _ = D.time_deinterleave(cifs, None if history is None else np.asarray(history, np.int8).reshape(15, nbits))
    decoded = np.asarray(decoded, np.uint8).reshape(cifs.shape[0], profile.nbytes)
    out = np.zeros((2, cifs.shape[0]), np.int64)
    for t in range(cifs.shape[0]):
        out[:, t] = count(logical[t, :profile.kept], coded_bits(decoded[t], profile))
    return out[0], out[1]
