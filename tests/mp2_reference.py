"""From-definition reference for following DAB (MPEG layer II) sub-channels: a restatement in plain Python of THE CONTRACT
at the top of include/dabgpu_mp2_frame.h (EN 300 401 7.3 / 7.4.1, ISO 11172-3 2.4.1 and Annex B).  Bit-serial: a frame
is turned into a list of bits, the CRC register is clocked one bit at a time, the tables are written out as lists.  It
shares no code with the header, with the kernels or with synth.mp2_frame (whose CRC goes through a byte table)."""
import struct

import numpy as np

ROW_BYTES = 220
MAGIC = 0x4332504D

RATES = {1: [None, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, None],
         0: [None, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, None]}
NBAL_48K_SMALL = [4, 4, 3, 3, 3, 3, 3, 3]
NBAL_48K_LARGE = [4] * 11 + [3] * 12 + [2] * 4
NBAL_24K = [4] * 4 + [3] * 7 + [2] * 19
MONO_ONLY, TWO_CHANNEL_ONLY = (32, 48, 56, 80), (224, 256, 320, 384)

GOOD, HEADER_ERROR, NO_CRC, CRC_FAILED = "good", "header", "no_crc", "crc"


def bits_of(data):
    return [(v >> (7 - k)) & 1 for v in bytes(data) for k in range(8)]


def number(bits):
    v = 0
    for b in bits:
        v = (v << 1) | b
    return v


def header(lf, B):
    """the header's fields when it is valid for B, else None: {id, protection, mode, mode_ext}"""
    b = bits_of(lf[:4])
    if len(b) < 32 or number(b[0:12]) != 0xFFF:
        return None
    ident, layer, protection = b[12], number(b[13:15]), b[15]
    index, sampling = number(b[16:20]), number(b[20:22])
    mode, mode_ext = number(b[24:26]), number(b[26:28])
    if layer != 2 or sampling != 1 or RATES[ident][index] != B:
        return None
    if ident == 1 and ((B in MONO_ONLY and mode != 3) or (B in TWO_CHANNEL_ONLY and mode == 3)):
        return None
    return {"id": ident, "protection": protection, "mode": mode, "mode_ext": mode_ext}


def crc_bit_serial(bits):
    reg = [1] * 16                                      # reg[0] = x^15 ... reg[15] = x^0
    for b in bits:
        fb = reg[0] ^ b
        reg = reg[1:] + [0]
        if fb:                                          # x^16 = x^15 + x^2 + 1
            reg[0] ^= 1
            reg[13] ^= 1
            reg[15] ^= 1
    return number(reg)


def shape(h, B):
    channels = 1 if h["mode"] == 3 else 2
    per_channel = B // channels
    if h["id"] == 1:
        nbal = NBAL_48K_SMALL if per_channel in (32, 48) else NBAL_48K_LARGE
        c = 2 if per_channel < 56 else 4
    else:
        nbal, c = NBAL_24K, 4
    bound = min((4, 8, 12, 16)[h["mode_ext"]], len(nbal)) if h["mode"] == 1 else len(nbal)
    return channels, nbal, bound, c


def check_frame(frame, B, want_id):
    """frame: its L bytes -> (kind, c)"""
    h = header(frame, B)
    if h is None or h["id"] != want_id:
        return HEADER_ERROR, 0
    channels, nbal, bound, c = shape(h, B)
    if h["protection"] == 1:
        return NO_CRC, c
    b = bits_of(frame)
    at, scfsi = 48, 0
    for sb, n in enumerate(nbal):
        fields = 2 if channels == 2 and sb < bound else 1
        for _ in range(fields):
            if at + n > len(b):
                return CRC_FAILED, c
            if number(b[at:at + n]) != 0:
                scfsi += 2 if channels == 2 and fields == 1 else 1
            at += n
    end = at + 2 * scfsi
    if end > len(b):
        return CRC_FAILED, c
    return (GOOD if crc_bit_serial(b[16:32] + b[48:end]) == number(b[32:48]) else CRC_FAILED), c


def pad_row(frame, c):
    L = len(frame)
    x = min(196, L - 8 - c)
    p = frame[L - 6 - c - (x - 4):L - 6 - c] + frame[L - 6:L - 2]
    assert len(p) == x
    row = bytes([0x80, x + 2]) + p + frame[L - 2:L] + bytes(2)
    return row + bytes(ROW_BYTES - len(row)), x


def read_carry(carry, B):
    """-> (synced, rate, [held frames])"""
    if carry is None:
        return 0, 0, []
    synced, held, rate, magic = struct.unpack("<4i", bytes(carry[:16]))
    ok = (magic == MAGIC and synced in (0, 1) and held in (0, 1) and rate in (0, 1, 2) and (synced == 1) == (rate != 0)
          and not (rate == 1 and held))
    if not ok:
        return 0, 0, []
    return synced, rate, [bytes(carry[16:16 + 3 * B])] * held


def carry_bytes(B):
    return (16 + 3 * B + 15) // 16 * 16


def follow(new_frames, B, carry=None):
    """One entry in one call.  new_frames: the n_cifs logical frames (bytes of 3 B each); carry: the record going in or
    None -> dict(rows [n][220] uint8, status [n][16] int32, follow (8 int32), result (16 int32), carry (bytes))."""
    synced, carry_rate, held = read_carry(carry, B)
    F = held + [bytes(f) for f in new_frames]
    T = len(F)
    heads = [header(f, B) for f in F]
    hits1 = sum(1 for h in heads if h and h["id"] == 1)
    votes0 = [sum(1 for i, h in enumerate(heads) if h and h["id"] == 0 and i % 2 == r) for r in (0, 1)]
    hits0 = sum(votes0)
    rate, phase, votes = 0, -1, 0
    if hits1 >= 1 and hits1 >= hits0:
        rate, phase, votes = 1, 0, hits1
    elif hits0 >= 1:
        rate, phase = 2, (1 if votes0[1] > votes0[0] else 0)
        votes = votes0[phase]
    elif synced:
        rate, phase = carry_rate, 0
    rows, status, counts, mode = [], [], {HEADER_ERROR: 0, NO_CRC: 0, CRC_FAILED: 0, GOOD: 0}, -1
    if rate == 0:
        kept = F[T - min(1, T):]
        dropped, synced_out = T - len(kept), 0
    else:
        per, want_id = (2, 0) if rate == 2 else (1, 1)
        n_rows = (T - phase) // per if T - phase >= per else 0
        for k in range(n_rows):
            frame = b"".join(F[phase + per * k:phase + per * k + per])
            kind, c = check_frame(frame, B, want_id)
            counts[kind] += 1
            if kind == GOOD:
                row, x = pad_row(frame, c)
                st = [1, 0, 0, 1, 1, 0, x + 6] + [0] * 9
            else:
                row, st = bytes(ROW_BYTES), [1, 0, 0, 1, 0, 0, 0] + [0] * 9
            rows.append(np.frombuffer(row, np.uint8))
            status.append(st)
        for i in range(phase, T, per):
            if heads[i] and heads[i]["id"] == want_id:
                mode = heads[i]["mode"]
                break
        kept = F[min(T, phase + per * n_rows):]
        dropped = phase
        synced_out = 1 if votes > 0 or n_rows == 0 else 0
    n = len(rows)
    record = struct.pack("<4i", synced_out, len(kept), rate if synced_out else 0, MAGIC) + b"".join(kept)
    record += bytes(carry_bytes(B) - len(record))
    hits = hits1 + hits0
    result = [{1: 1, 2: 0, 0: -1}[rate], {1: 48000, 2: 24000, 0: 0}[rate], B if rate else 0, mode if rate else -1, phase, len(kept),
              synced_out, hits, n, counts[HEADER_ERROR], counts[CRC_FAILED], counts[NO_CRC], dropped, 0, 0, 0]
    return {"rows": np.stack(rows) if rows else np.zeros((0, ROW_BYTES), np.uint8),
            "status": np.array(status, np.int32).reshape(n, 16),
            "follow": np.array([n, phase, synced_out, dropped, hits, len(kept), 0, 0], np.int32),
            "result": np.array(result, np.int32), "carry": record}
