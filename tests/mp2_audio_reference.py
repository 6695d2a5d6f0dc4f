"""From-definition reference for layer-II frames taken on to sub-band samples and audio levels: a restatement in plain
Python of THE CONTRACT at the top of include/dabgpu_mp2_audio.h (ISO 11172-3 2.4.1.6, 2.4.2.6, 2.4.3.3, Annex B tables B.2
and B.4; ISO 13818-3 table B.1).  Bit-serial: a frame is a list of bits read one field after the other in stream order;
the tables are written out as lists.  Values come twice: in np.float32, operation for operation as the contract words
them (the bit-exact form), and in float64 from the definition (2 s + 1 - n) / n * 2^(1 - i / 3).  It shares no code with
the header, with the kernel or with synth; header fields and the GOOD check are those of tests/mp2_reference.py."""
import numpy as np

import mp2_reference as M

DECODED, NOT_GOOD, OVERRUN = 0, 1, 2

#: levels of allocation index 1, 2, ... per sub-band
LEVELS_48K_LARGE = (
    [[3, 7, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383, 32767, 65535]] * 3
    + [[3, 5, 7, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 65535]] * 8
    + [[3, 5, 7, 9, 15, 31, 65535]] * 12
    + [[3, 5, 65535]] * 4)
LEVELS_48K_SMALL = (
    [[3, 5, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383, 32767]] * 2
    + [[3, 5, 9, 15, 31, 63, 127]] * 6)
LEVELS_24K = (
    [[3, 5, 7, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383]] * 4
    + [[3, 5, 9, 15, 31, 63, 127]] * 7
    + [[3, 5, 9]] * 19)
GROUPED = {3: 5, 5: 7, 9: 10}                          # levels -> bits of the code word of three samples
SAMPLE_BITS = {7: 3, 15: 4, 31: 5, 63: 6, 127: 7, 255: 8, 511: 9, 1023: 10, 2047: 11, 4095: 12, 8191: 13, 16383: 14,
               32767: 15, 65535: 16}
#: SCFSI -> which of the indices sent holds in parts 0, 1, 2
PARTS = {0: [0, 1, 2], 1: [0, 0, 1], 2: [0, 0, 0], 3: [0, 1, 1]}
SENT = {0: 3, 1: 2, 2: 1, 3: 2}

_C = [2.0, 2.0 ** (2.0 / 3.0), 2.0 ** (1.0 / 3.0)]


def scale32(i):
    """S[i] as the contract computes it: (float)C[i % 3] scaled exactly by 2^-(i / 3); 0 for the forbidden 63"""
    if i == 63:
        return np.float32(0.0)
    return np.float32(np.float32(_C[i % 3]) * np.float32(2.0 ** -(i // 3)))


def scale64(i):
    return 0.0 if i == 63 else 2.0 ** (1.0 - i / 3.0)


def levels_table(h, B):
    channels = 1 if h["mode"] == 3 else 2
    if h["id"] == 0:
        return LEVELS_24K
    return LEVELS_48K_SMALL if B // channels in (32, 48) else LEVELS_48K_LARGE


def decode(frame, B, want_id):
    """One frame the follow call found GOOD -> dict(kind, channels, cells, scf63, v32 float32 [2][36][32], v64 float64
    [2][36][32], classes {(sb, ch): n}, E or None, limit)"""
    out = dict(kind=NOT_GOOD, channels=0, cells=0, scf63=0, v32=np.zeros((2, 36, 32), np.float32), v64=np.zeros((2, 36, 32)),
               classes={}, E=None, limit=None)
    h = M.header(frame, B)
    if h is None or h["id"] != want_id:
        return out
    channels, nbal, bound, c = M.shape(h, B)
    table = levels_table(h, B)
    assert len(table) == len(nbal) and all(len(row) == 2 ** n - 1 for row, n in zip(table, nbal))
    bits = M.bits_of(frame)
    limit = 8 * (len(frame) - 6 - c)
    out["limit"], out["kind"] = limit, OVERRUN
    at = 48
    # allocation: one field per channel below the bound, one for both at or above it
    alloc = {}
    for sb, n in enumerate(nbal):
        shared = channels == 2 and sb >= bound
        for ch in range(1 if shared else channels):
            if at + n > limit:
                return out
            a = M.number(bits[at:at + n])
            at += n
            for to in ((0, 1) if shared else (ch,)):
                alloc[(sb, to)] = a
    cells = [(sb, ch) for sb in range(len(nbal)) for ch in range(channels) if alloc[(sb, ch)]]
    scfsi = {}
    for cell in cells:
        if at + 2 > limit:
            return out
        scfsi[cell] = M.number(bits[at:at + 2])
        at += 2
    index, scf63 = {}, 0
    for cell in cells:
        sent = []
        for _ in range(SENT[scfsi[cell]]):
            if at + 6 > limit:
                return out
            sent.append(M.number(bits[at:at + 6]))
            at += 6
        scf63 += sent.count(63)
        index[cell] = [sent[j] for j in PARTS[scfsi[cell]]]
    classes = {(sb, ch): table[sb][alloc[(sb, ch)] - 1] for sb, ch in cells}
    fields = [(sb, ch) for sb in range(len(nbal)) for ch in range(1 if channels == 2 and sb >= bound else channels) if alloc[(sb, ch)]]
    granule = sum(GROUPED[classes[f]] if classes[f] in GROUPED else 3 * SAMPLE_BITS[classes[f]] for f in fields)
    out["E"] = at + 12 * granule
    if out["E"] > limit:
        return out
    s = {cell: [] for cell in cells}
    for g in range(12):
        for sb, ch in fields:
            n = classes[(sb, ch)]
            if n in GROUPED:
                code = M.number(bits[at:at + GROUPED[n]])
                at += GROUPED[n]
                three = [code % n, (code // n) % n, (code // (n * n)) % n]
            else:
                b = SAMPLE_BITS[n]
                three = [M.number(bits[at + k * b:at + (k + 1) * b]) for k in range(3)]
                at += 3 * b
            for to in ((0, 1) if channels == 2 and sb >= bound else (ch,)):
                s[(sb, to)] += three
    assert at == out["E"]
    for (sb, ch), codes in s.items():
        n = classes[(sb, ch)]
        num = 2 * np.array(codes, np.int64) + 1 - n
        f32 = np.repeat(np.array([scale32(i) for i in index[(sb, ch)]], np.float32), 12)
        f64 = np.repeat(np.array([scale64(i) for i in index[(sb, ch)]], np.float64), 12)
        out["v32"][ch, :, sb] = (num.astype(np.float32) * np.float32(1.0 / n)) * f32
        out["v64"][ch, :, sb] = num / n * f64
    assert out["v32"].dtype == np.float32
    out.update(kind=DECODED, channels=channels, cells=len(cells), scf63=scf63, classes=classes)
    return out


def level(dec):
    """the level record of one decoded frame: (kind, channels, cells, scf63, power float64 [2] from the definition, peak
    float32 [2] exact)"""
    return (dec["kind"], dec["channels"], dec["cells"], dec["scf63"], (dec["v64"] ** 2).sum(axis=(1, 2)),
            np.abs(dec["v32"]).max(axis=(1, 2)))


def subbands(new_frames, B, carry, followed):
    """One entry in one call, behind mp2_reference.follow (followed = what it returned for the same frames and carry):
    -> (list of decode() results, one per row, and the counters [decoded, not_good, overrun, silent])"""
    _synced, _rate, held = M.read_carry(carry, B)
    F = held + [bytes(f) for f in new_frames]
    ident, phase, n = int(followed["result"][0]), int(followed["result"][4]), int(followed["result"][8])
    rows, tally = [], [0, 0, 0, 0]
    for k in range(n):
        per = 1 if ident == 1 else 2
        frame = b"".join(F[phase + per * k:phase + per * k + per])
        if followed["status"][k][4] == 1:
            dec = decode(frame, B, ident)
        else:
            dec = decode(b"", B, ident)
        rows.append(dec)
        tally[dec["kind"]] += 1
        tally[3] += dec["kind"] == DECODED and float((dec["v32"].astype(np.float64) ** 2).sum()) == 0.0
    return rows, tally
