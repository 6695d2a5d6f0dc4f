"""The transmitted signal of include/dabgpu.h, "ETI(NI) to IQ", composed from dabgpu.synth (an independent restatement of
the transmit side of EN 300 401): fic_encode, msc_encode_lf with eep_mask / uep_mask, time_interleave(cyclic=False),
modulate_frame and tii_null.  No device, nothing of the library; float64 inside, complex64 out.

A sub-channel is a dict {id, start, bitrate, uep (bool), eep_type (0 = A, 1 = B), level (1..)} as in eti_reference.
"""
import numpy as np

from dabgpu import synth

import eti_reference as E

BAD_INPUT, MISALIGNED = 1, 2


def mask_of(st):
    """-> (puncture mask, size in capacity units)."""
    if st["uep"]:
        return synth.uep_mask(synth.uep_index(st["bitrate"], st["level"]))
    return synth.eep_mask(st["eep_type"], st["level"], st["bitrate"])


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


def frame_bits(streams, fibs, data, refused=()):
    """The 230 400 bits of every transmission frame of ONE stream that starts with CIF 0 -> uint8 [n_cif / 4][230400].
    refused: the ETI frames that are not taken; they are modulated as 96 zero FIC bytes and zero stream bytes."""
    fibs = np.array(fibs, np.uint8).reshape(-1, 3, 32)
    n_cif = fibs.shape[0]
    assert n_cif % 4 == 0
    refused = set(refused)
    for t in refused:
        fibs[t] = 0
    cifs = np.zeros((n_cif, synth.NB_CIF_BITS), np.uint8)
    for st in streams:
        mask, size_cu = mask_of(st)
        d = np.array(data[st["id"]], np.uint8)
        for t in refused:
            d[t] = 0
        coded = np.zeros((n_cif, 64 * size_cu), np.uint8)
        for r in range(n_cif):
            c = synth.msc_encode_lf(d[r], mask)
            coded[r, :c.size] = c                              # (UEP padding bits stay 0)
        a = 64 * st["start"]
        cifs[:, a:a + 64 * size_cu] = synth.time_interleave(coded, cyclic=False)
    bits = np.zeros((n_cif // 4, synth.NB_FRAME_BITS), np.uint8)
    for f in range(n_cif // 4):
        bits[f, :synth.NB_FIC_BITS] = synth.fic_encode(fibs[4 * f:4 * f + 4].reshape(12, 32))
        bits[f, synth.NB_FIC_BITS:] = cifs[4 * f:4 * f + 4].ravel()
    return bits


def modulate(bits, tii=None, gain=1.0):
    """frame bits [n][230400] -> complex64 [n][196608]; tii = (sub c, main p) or None."""
    frames = [synth.modulate_frame(b, None if tii is None else [tii]).astype(np.complex128) * gain for b in bits]
    return np.stack(frames).astype(np.complex64)


def status(eti, refused=()):
    """[(flags, refused mask)] per transmission frame: eti [n_cif][6144]."""
    out = []
    for f in range(len(eti) // 4):
        m = sum(1 << j for j in range(4) if 4 * f + j in set(refused))
        fp = int(eti[4 * f][6]) >> 5
        out.append(((BAD_INPUT if m else 0) | (MISALIGNED if fp % 4 else 0), m))
    return out
