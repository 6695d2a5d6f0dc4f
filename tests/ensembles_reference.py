"""Ensembles with their own multiplexes, for the tests of dabgpu_decode_ensembles_dev and dabgpu_fig_subchannels: a cyclic
multiplex with any mix of EEP-A, EEP-B and UEP sub-channels composed from dabgpu.synth's pieces, its frames as soft bits
(clean, or with the noise tests/test_uep.py puts on them), and what the oracle decodes from soft bits.  TEST
INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import dabgpu
from dabgpu import synth
from oracle import oracle as O

NB_FIC_BITS, NB_CIF_BITS = synth.NB_FIC_BITS, synth.NB_CIF_BITS


@functools.lru_cache(maxsize=None)
def _prbs(n):
    return synth.prbs(n)


def descriptor(spec):
    """spec: ("eep", option, level, bitrate, start_cu) or ("uep", table_index, start_cu) -> dabgpu.Subchannel"""
    if spec[0] == "uep":
        return dabgpu.uep_subchannel(spec[1], spec[2])
    return dabgpu.subchannel(spec[4], spec[3], level=spec[2], eep_type=spec[1])


def oracle_code(spec):
    """-> (mask, kept, nsteps) of the oracle's own tables"""
    if spec[0] == "uep":
        return O.uep_puncture_mask(spec[1])[:3]
    return O.eep_puncture_mask(spec[1], spec[2], spec[3])[:3]


class Multiplex:
    """`n_cycle` frames (4 n_cycle CIFs) that tile into a continuous transmission: random FIBs, the sub-channels of `specs`
    with random bytes (msc_bytes[k][r]: logical frame r of sub-channel k), random filler elsewhere."""

    def __init__(self, seed, specs, n_cycle=4):
        rng = np.random.default_rng(seed)
        self.specs, self.n_cycle = list(specs), n_cycle
        R = 4 * n_cycle
        self.fibs = synth.make_fibs(rng, 12 * n_cycle).reshape(n_cycle, 12, 32)
        cifs = rng.integers(0, 2, size=(R, NB_CIF_BITS), dtype=np.uint8)
        self.scs, self.msc_bytes = [], []
        for spec in self.specs:
            sc = descriptor(spec)
            mask = (synth.uep_mask(spec[1]) if spec[0] == "uep" else synth.eep_mask(spec[1], spec[2], spec[3]))[0].astype(bool)
            data = rng.integers(0, 256, size=(R, sc.bitrate_kbps * 3), dtype=np.uint8)
            coded = np.zeros((R, sc.length * 64), np.uint8)           # (UEP: padding zeros behind the codeword)
            for r in range(R):
                bits = np.unpackbits(data[r])
                cw = synth.conv_encode(bits ^ _prbs(bits.size))[mask]
                coded[r, :cw.size] = cw
            cifs[:, sc.start_address * 64:(sc.start_address + sc.length) * 64] = synth.time_interleave(coded, cyclic=True)
            self.scs.append(sc)
            self.msc_bytes.append(data)
        self.frame_bits = np.zeros((n_cycle, synth.NB_FRAME_BITS), np.uint8)
        for f in range(n_cycle):
            self.frame_bits[f, :NB_FIC_BITS] = synth.fic_encode(self.fibs[f])
            self.frame_bits[f, NB_FIC_BITS:] = cifs[4 * f:4 * f + 4].ravel()

    def frames(self, n_frames, first=0):
        """bits of frames first .. first + n_frames - 1 of the endless transmission"""
        return self.frame_bits[(first + np.arange(n_frames)) % self.n_cycle]

    def soft(self, n_frames, first=0, rng=None):
        """the same as soft bits: +-127, with uniform noise of +-90 when `rng` is given (the level of tests/test_uep.py, at
        which the oracle still decodes every profile used here)"""
        s = np.where(self.frames(n_frames, first) > 0, 127, -127).astype(np.int16)
        if rng is not None:
            s = s + rng.integers(-90, 91, s.shape)
        return np.clip(s, -127, 127).astype(np.int8)

    def sent(self, k, t, first=0):
        """bytes of sub-channel k that CIF t of a stream starting at frame `first` completes (sent 15 CIFs earlier)"""
        return self.msc_bytes[k][(4 * first + t - 15) % (4 * self.n_cycle)]


def cif_rows(soft, sc):
    """soft [n_frames][230400] -> the sub-channel's part of every CIF, [4 n_frames][length * 64]"""
    n = soft.shape[0]
    return soft[:, NB_FIC_BITS:].reshape(4 * n, NB_CIF_BITS)[:, sc.start_address * 64:(sc.start_address + sc.length) * 64]


def oracle_subchannel(soft, spec, hist_in=None):
    """what the oracle decodes from one stream's frames: out [4 n_frames][bytes], history_out [15][bits]"""
    sc = descriptor(spec)
    mask, kept, nsteps = oracle_code(spec)
    rows = cif_rows(soft, sc)
    padded = np.concatenate([np.zeros((15, rows.shape[1]), np.int8) if hist_in is None else hist_in, rows])
    out = np.stack([O.msc_decode_lf(O.time_deinterleave(padded[t:t + 16])[:kept], mask, nsteps) for t in range(rows.shape[0])])
    return out, padded[-15:]


def oracle_fic(soft):
    """-> fib [n_frames][12][32], crc_ok [n_frames][12]"""
    fibs, oks = [], []
    for f in range(soft.shape[0]):
        fib, ok = O.fic_decode(soft[f, :NB_FIC_BITS])
        fibs.append(np.asarray(fib).reshape(12, 32))
        oks.append(np.asarray(ok))
    return np.stack(fibs), np.stack(oks)
