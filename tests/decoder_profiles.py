"""The inputs of tests/test_decoder_profiles.py: every protection profile the sweep covers, 16 chosen punctured codewords
for each, the nine packed streams that carry them, the exact reference's answers and the mutant decoders the sensitivity
tests hold the sweep to.  Imports numpy and decoder_reference alone: nothing here comes from the library or the oracle.

Profiles (88): all 64 UEP rows, EEP-A levels 1..4 at 8, 16, 24 and 72 kbit/s (n = 1 with its special case at level 2, even,
odd, larger), EEP-B levels 1..4 at 32 and 96 kbit/s.  A profile's key is ("uep", row, 0, 0) or ("eep", option, level, rate).

Codewords.  c [16][kept] int8 per profile: 0 a saturated clean codeword of a random message, 1 of the all-ones message
(the headroom excursion), 2 and 3 signal at amplitude 60 with Gaussian noise at 4 dB, 4..9 uniform in -127..127, 10..15 on
the 16-level grid 16 k + 8 (many exact ties).  The noise codewords are what makes the sweep see a single lost soft bit:
the code corrects a lost bit of a signal codeword, but the optimum of a noise codeword moves with it.

Streams.  The sub-channel's CIFs are cyclic with period 16: the logical frame that is complete with CIF t is c[t mod 16],
so CIF q carries, at bit i, c[(q - 1 - delay(i)) mod 16][i] -- built by decoder_reference.time_interleave, not by that
formula.  Four frames (16 CIFs) are one period, history_in is the 15 CIFs before them in the same cycle (rows 1..15 of
the period), history_out must be the same rows, and codeword t of any longer run is c[t mod 16].  Padding bits of UEP
sub-channels, unused capacity units and the FIC hold uniform noise.  The profiles are packed first-fit by decreasing size
into streams of 864 capacity units; inside a stream the UEP rows with padding come first, so that each is followed directly
by another entry, every stream starts at CU 0, and where capacity is left over the last entry is moved to end at CU 864."""
import functools

import numpy as np

import decoder_reference as R

N_CW = 16
NB_FRAME_BITS = 230400
PROFILES = tuple([("uep", i, 0, 0) for i in range(64)]
                 + [("eep", 0, lv, br) for br in (8, 16, 24, 72) for lv in (1, 2, 3, 4)]
                 + [("eep", 1, lv, br) for br in (32, 96) for lv in (1, 2, 3, 4)])
CLEAN, SIGNAL, NOISE = (0, 1), (2, 3), tuple(range(4, 16))


def name(key):
    return "uep%d" % key[1] if key[0] == "uep" else "eep%d%s-%d" % (key[2], "AB"[key[1]], key[3])


@functools.lru_cache(maxsize=None)
def profile(key):
    return R.uep_profile(key[1]) if key[0] == "uep" else R.eep_profile(key[1], key[2], key[3])


def block_pis(p):
    """The puncturing index of every 32-step block of the profile, in order."""
    return [pi for n, pi in p.blocks for _ in range(n)]


def mask_of(pis, tail=R.V_TAIL):
    return np.concatenate([np.tile(R.V_PI[pi - 1], 4) for pi in pis] + [tail])


LENGTHS = tuple(sorted({profile(k).nsteps for k in PROFILES}))
SHORT_LENGTHS = tuple(n for n in LENGTHS if n <= 1158)           # the single-bit study's profiles


def keys_of_length(nsteps):
    return [k for k in PROFILES if profile(k).nsteps == nsteps]


def _seed(key, salt):
    return [("uep", "eep").index(key[0]), key[1], key[2], key[3], salt]


# ------------------------------------------------------------------------------------------------ packing
@functools.lru_cache(maxsize=None)
def streams():
    """-> tuple of streams, each a tuple of (key, start CU) in address order."""
    bins = []
    for k in sorted(PROFILES, key=lambda k: (-profile(k).size_cu, PROFILES.index(k))):
        for b in bins:
            if sum(profile(x).size_cu for x in b) + profile(k).size_cu <= 864:
                b.append(k)
                break
        else:
            bins.append([k])
    out = []
    for b in bins:
        order = [k for k in b if profile(k).padding] + [k for k in b if not profile(k).padding]
        at, placed = 0, []
        for k in order:
            placed.append([k, at])
            at += profile(k).size_cu
        if at < 864 and len(order) >= 2 and not profile(order[-2]).padding:
            placed[-1][1] = 864 - profile(order[-1]).size_cu             # the gap lies in front of the last entry
        out.append(tuple((k, s) for k, s in placed))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def place(key):
    """-> (stream, position in the stream's list, start CU)"""
    for s, lst in enumerate(streams()):
        for j, (k, start) in enumerate(lst):
            if k == key:
                return s, j, start
    raise KeyError(key)


# ------------------------------------------------------------------------------------------------ codewords
@functools.lru_cache(maxsize=None)
def codewords(key):
    """-> c int8 [16][kept], the messages of the two clean codewords uint8 [2][nsteps - 6] (encoder input)."""
    p = profile(key)
    rng = np.random.default_rng(_seed(key, 0xC0DE))
    sent = np.flatnonzero(p.mask)
    msgs = rng.integers(0, 2, (4, p.nsteps - 6), dtype=np.uint8)
    msgs[1] = 1
    code = (R.conv_encode(msgs).astype(np.int64) * 2 - 1)[:, sent]
    c = np.zeros((N_CW, p.kept), np.int64)
    c[0:2] = code[0:2] * 127
    sigma = 60 / 10.0 ** (4.0 / 20.0)
    c[2:4] = np.clip(np.rint(code[2:4] * 60 + rng.normal(0.0, sigma, code[2:4].shape)), -127, 127)
    c[4:10] = rng.integers(-127, 128, (6, p.kept))
    c[10:16] = rng.integers(-8, 8, (6, p.kept)) * 16 + 8
    c = c.astype(np.int8)
    c.setflags(write=False)
    return c, msgs[:2]


@functools.lru_cache(maxsize=None)
def period(key):
    """The sub-channel's 16 CIFs int8 [16][64 size_cu]: CIF q of the cyclic transmission is row q mod 16."""
    p = profile(key)
    c, _ = codewords(key)
    nbits = 64 * p.size_cu
    lf = np.zeros((N_CW, nbits), np.int8)
    lf[:, :p.kept] = c
    sent = lf[(np.arange(48) + 15) % 16]                 # the frame that STARTS with CIF r is complete with CIF r + 15
    cifs = R.time_interleave(sent)[16:32].copy()         # CIFs 16 .. 31: every frame that reaches them is among the 48
    if p.padding:
        cifs[:, p.kept:] = np.random.default_rng(_seed(key, 0xBAD)).integers(-127, 128, (16, p.padding))
    cifs.setflags(write=False)
    return cifs


def history(key):
    """history_in of the four frames, and what history_out must be: the 15 CIFs before CIF 0 = the last 15 of the period."""
    return period(key)[1:]


@functools.lru_cache(maxsize=None)
def stream_frames(s):
    """Four whole frames int8 [4][230400] of stream s: uniform noise in the FIC and in every capacity unit no entry uses."""
    rng = np.random.default_rng([s, 0x57EA])
    soft = rng.integers(-127, 128, (4, NB_FRAME_BITS), dtype=np.int8)
    cifs = soft[:, R.NB_FIC_BITS:].reshape(16, R.NB_CIF_BITS)
    for k, start in streams()[s]:
        cifs[:, 64 * start:64 * (start + profile(k).size_cu)] = period(k)
    soft[:, R.NB_FIC_BITS:] = cifs.reshape(4, 4 * R.NB_CIF_BITS)
    soft.setflags(write=False)
    return soft


@functools.lru_cache(maxsize=None)
def fic_ref(s):
    return R.fic_reference(stream_frames(s))


@functools.lru_cache(maxsize=None)
def ber_bytes(key):
    """Random "decoded" bytes uint8 [16][nbytes] for the channel BER: the count must not depend on a decoder."""
    return np.random.default_rng(_seed(key, 0xBE2)).integers(0, 256, (N_CW, profile(key).nbytes), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the reference's answers
@functools.lru_cache(maxsize=None)
def length_ref(nsteps):
    """One viterbi call for every profile of this length, their codewords stacked as lanes."""
    keys = keys_of_length(nsteps)
    mother = np.concatenate([R.depuncture(codewords(k)[0], profile(k).mask) for k in keys])
    d = R.viterbi(mother, stats=False)
    d.bits()
    return keys, mother, d


@functools.lru_cache(maxsize=None)
def ref(key):
    """-> mother int64 [16][4 nsteps], Decoded of the 16 codewords."""
    keys, mother, d = length_ref(profile(key).nsteps)
    i = keys.index(key)
    return mother[N_CW * i:N_CW * (i + 1)], d.lanes(np.arange(N_CW * i, N_CW * (i + 1)))


def reference_bytes(mother):
    """What the reference returns for mother soft bits [B][4 nsteps] as an MSC decoder (energy dispersal undone)."""
    bits = R.viterbi(mother, stats=False).bits()
    return np.packbits(bits ^ R.prbs(bits.shape[1])[None, :], axis=1)


# ------------------------------------------------------------------------------------------------ structural mutants
STRUCTURAL = ("first block longer", "one block's PI", "tail shifted", "one bit late", "padding as data")


def _logical(key, late=0):
    """The 16 logical frames as a decoder reads them that takes the sub-channel `late` bits behind its start."""
    s, _, start = place(key)
    nbits = 64 * profile(key).size_cu
    cifs = stream_frames(s)[:, R.NB_FIC_BITS:].reshape(16, R.NB_CIF_BITS)
    cifs = np.concatenate([cifs, np.zeros((16, late), np.int8)], axis=1)[:, 64 * start + late:64 * start + late + nbits]
    return R.time_deinterleave(cifs, cifs[1:])


def noise_ref(key):
    """ref(key) of the 12 noise codewords alone, which is what the mutants are decoded on: a mutant their bytes give away
    is given away by the 16, so judging by them only makes the sensitivity tests' conditions harder to meet."""
    mother, d = ref(key)
    return mother[list(NOISE)], d.lanes(np.array(NOISE))


def mutant_mother(key, kind):
    """The mother soft bits [12][4 nsteps] a decoder with one wrong table entry sees for the 12 noise codewords (None:
    the mutant does not exist for this profile)."""
    p = profile(key)
    rows = _logical(key, 1 if kind == "one bit late" else 0)[0].astype(np.int64)
    pis, tail = block_pis(p), R.V_TAIL
    if kind == "first block longer":                     # the first region takes the next region's first block
        first = pis[0]
        pis[[pi != first for pi in pis].index(True)] = first
    elif kind == "one block's PI":
        b = int(np.random.default_rng(_seed(key, 0xB10C)).integers(0, len(pis)))
        pis[b] += 1 if pis[b] < 24 else -1
    elif kind == "tail shifted":
        tail = np.roll(R.V_TAIL, 1)
    elif kind == "padding as data":                      # the 12 tail bits taken from the END of the sub-channel
        if not p.padding:
            return None
        rows = np.concatenate([rows[:, :p.kept - 12], rows[:, -12:]], axis=1)
    mask = mask_of(pis, tail)
    assert mask.size == p.mask.size and ((mask != p.mask).any() or kind in ("one bit late", "padding as data"))
    kept = int(mask.sum())
    rows = np.concatenate([rows, np.zeros((N_CW, max(0, kept - rows.shape[1])), np.int64)], axis=1)
    return R.depuncture(rows[list(NOISE), :kept], mask)


# ------------------------------------------------------------------------------------------------ single-bit mutants
def single_bit_positions(key):
    """Indices into the punctured codeword: the first and last kept bit of each puncturing region and of the tail, the
    kept bits on either side of every eighth 24-step tile boundary, and 4 seeded random ones.  (With every fourth boundary
    and 8 random ones the module's CPU part took 39.9 s, above its allowance; the shares were 3.6 / 0 / 6.8 / 5.8 / 2.8 %.)"""
    p = profile(key)
    upto = np.concatenate([[0], np.cumsum(p.mask.reshape(-1, 4).sum(axis=1))])       # kept bits in front of each step
    pos, step = [], 0
    for n, _pi in p.blocks:
        if n > 0:
            pos += [int(upto[step]), int(upto[step + 32 * n]) - 1]
            step += 32 * n
    pos += [int(upto[step]), p.kept - 1]
    for t in range(192, p.nsteps, 192):
        pos += [int(upto[t]) - 1, int(upto[t])]
    pos += np.random.default_rng(_seed(key, 0xB17)).integers(0, p.kept, 4).tolist()
    return sorted(set(pos))


def _neighbour(p, j):
    """The kept bit that bit j is exchanged with: the next one (the one before for the last).  All coded bits of the first
    step are equal (the register holds the new bit alone and every generator has its first tap set) and so are those of
    the last step (the oldest bit alone, every generator has its last tap set): exchanging two bits inside either step
    changes no codeword's metric, it is no error a test could see.  There the partner comes from the adjacent step."""
    step = np.flatnonzero(p.mask) // 4                   # the trellis step of every kept bit
    k = j + 1 if j + 1 < p.kept else j - 1
    if step[j] == step[k] == 0:
        k = int(np.flatnonzero(step == 1)[0])
    elif step[j] == step[k] == p.nsteps - 1:
        k = int(np.flatnonzero(step == p.nsteps - 2)[-1])
    return k


def single_bit_mutants(key):
    """-> labels, mother int64 [mutants][12][4 nsteps]: what a decoder sees whose table loses one kept soft bit (erased)
    or exchanges it with its neighbour (see _neighbour), in every codeword at once.  Only the 12 noise codewords are
    decoded: a mutant their bytes give away is given away by the 16, so the share that passes can only be overstated."""
    p = profile(key)
    c = codewords(key)[0][list(NOISE)].astype(np.int64)
    labels, rows = [], []
    for j in single_bit_positions(key):
        x = c.copy()
        x[:, j] = 0
        labels.append("bit %d erased" % j); rows.append(x)
        k = _neighbour(p, j)
        x = c.copy()
        x[:, [j, k]] = x[:, [k, j]]
        labels.append("bits %d and %d exchanged" % (j, k)); rows.append(x)
    mother = R.depuncture(np.concatenate(rows), p.mask)
    return labels, mother.reshape(len(labels), len(NOISE), -1)
