"""ETI(NI) frames from the definition (include/dabgpu.h, "ETI(NI) output"): a writer and a
reader in plain Python, byte by byte, sharing nothing with the library or its binding but synth.crc16.

A stream is a dict {id, start, bitrate, uep (bool), eep_type (0 = A, 1 = B), level (1..)}.  All multi-bit fields are
big-endian, MSB first; one frame is 6144 bytes:

    ERR(1) FSYNC(3) | FCT(1) FICF:1 NST:7 FP:3 MID:2 FL:11 | NST x [SCID:6 SAD:10 TPL:6 STL:10] | MNSC(2) CRC(2) |
    FIC(96) | streams by ascending SAD, 8 STL bytes each | CRC(2) RFU(2) | TIST(4) | 0x55 ...
"""
from dabgpu.synth import crc16

FRAME_BYTES = 6144
FSYNC_EVEN, FSYNC_ODD = bytes([0x07, 0x3A, 0xB6]), bytes([0xF8, 0xC5, 0x49])


def _bits(*fields):
    v, n = 0, 0
    for val, w in fields:
        if not 0 <= val < (1 << w):
            raise ValueError("field %d does not fit %d bits" % (val, w))
        v, n = (v << w) | val, n + w
    assert n % 8 == 0
    return v.to_bytes(n // 8, "big")


def tpl_of(st):
    if st["uep"]:
        return 0x10 | (st["level"] - 1)
    return 0x20 | (st["eep_type"] << 2) | (st["level"] - 1)


def stl_of(st):
    if st["bitrate"] % 8:
        raise ValueError("bit rate not a multiple of 8")
    return st["bitrate"] * 3 // 8


def ordered(streams):
    return sorted(streams, key=lambda st: st["start"])


def frame_length(streams):
    """FL (32-bit words of STC + MNSC/CRC + FIC + stream data) and the bytes before the padding."""
    fl = len(streams) + 1 + 24 + 2 * sum(stl_of(st) for st in streams)
    return fl, 4 * fl + 16


def write_frame(streams, cif_count, fic, data, err):
    """One frame.  fic: 96 bytes; data: {stream id: the stream's bytes of this CIF (bitrate * 3)}; cif_count 0..4999;
    err: the ERR byte."""
    streams = ordered(streams)
    upper, lower = cif_count // 250, cif_count % 250
    fl, length = frame_length(streams)
    if length > FRAME_BYTES or len(streams) > 64:
        raise ValueError("does not fit an ETI frame")
    fct, fp = lower, (upper * 250 + lower) % 8
    fc = _bits((fct, 8), (1, 1), (len(streams), 7), (fp, 3), (1, 2), (fl, 11))
    stc = b"".join(_bits((st["id"], 6), (st["start"], 10), (tpl_of(st), 6), (stl_of(st), 10)) for st in streams)
    head = fc + stc + b"\xff\xff"
    head += crc16(head).to_bytes(2, "big")
    fic = bytes(fic)
    assert len(fic) == 96
    mst = fic
    for st in streams:
        d = bytes(data[st["id"]])
        assert len(d) == 8 * stl_of(st), (st, len(d))
        mst += d
    eof = crc16(mst).to_bytes(2, "big") + b"\xff\xff"
    frame = bytes([err]) + (FSYNC_ODD if fct & 1 else FSYNC_EVEN) + head + mst + eof + b"\xff\xff\xff\xff"
    assert len(frame) == length
    return frame + b"\x55" * (FRAME_BYTES - length)


def err_byte(crc_ok3, warmup=False):
    return 0x00 if warmup else (0xFF if all(crc_ok3) else 0xE1)


def read_frame(frame):
    """Parse and check one frame -> dict; ValueError names what is wrong."""
    f = bytes(frame)
    if len(f) != FRAME_BYTES:
        raise ValueError("length")
    fct = f[4]
    if f[1:4] not in (FSYNC_EVEN, FSYNC_ODD) or (f[1:4] == FSYNC_ODD) != bool(fct & 1):
        raise ValueError("fsync")
    ficf, nst = f[5] >> 7, f[5] & 0x7F
    fp, mid, fl = f[6] >> 5, (f[6] >> 3) & 3, ((f[6] & 7) << 8) | f[7]
    if ficf != 1 or mid != 1 or nst > 64:
        raise ValueError("header")
    streams, pos = [], 8
    for _ in range(nst):
        w = int.from_bytes(f[pos:pos + 4], "big")
        streams.append({"scid": w >> 26, "sad": (w >> 16) & 0x3FF, "tpl": (w >> 10) & 0x3F, "stl": w & 0x3FF})
        pos += 4
    if fl != nst + 1 + 24 + 2 * sum(s["stl"] for s in streams) or 4 * fl + 16 > FRAME_BYTES:
        raise ValueError("fl")
    mnsc = f[pos:pos + 2]
    if int.from_bytes(f[pos + 2:pos + 4], "big") != crc16(f[4:pos + 2]):
        raise ValueError("header crc")
    pos += 4
    start = pos
    fic = f[pos:pos + 96]
    pos += 96
    for s in streams:
        s["data"] = f[pos:pos + 8 * s["stl"]]
        pos += 8 * s["stl"]
    if int.from_bytes(f[pos:pos + 2], "big") != crc16(f[start:pos]):
        raise ValueError("data crc")
    return {"err": f[0], "fct": fct, "fp": fp, "nst": nst, "fl": fl, "length": 4 * fl + 16, "mnsc": mnsc, "fic": fic,
            "streams": streams, "rfu": f[pos + 2:pos + 4], "tist": f[pos + 4:pos + 8], "padding": f[pos + 8:]}


def fig0_0_count(fib, crc_ok):
    """The CIF count a valid FIB that begins with FIG 0/0 carries, else None."""
    fib = bytes(fib)
    if not crc_ok or fib[0] != 0x05 or fib[1] != 0x00:
        return None
    upper, lower = fib[4] & 0x1F, fib[5]
    if upper >= 20 or lower >= 250:
        return None
    return upper * 250 + lower


WARMUP, FIB_CRC, NO_ANCHOR, COUNT_MISMATCH = 1, 2, 4, 8


def history_of_record(fib, crc_ok, next_count, valid):
    """The history a dabgpu_eti_history record stands for, whatever the caller left in it (include/dabgpu.h, the record's
    comment): `valid` below 0 counts as 0 and above 15 as 15, the newest `valid` of the 15 slots hold a CIF, next_count is
    the int32 read as unsigned (write_stream takes it modulo 5000) and means nothing when valid is 0.
    fib [15][96], crc_ok [15][3] -> the dict write_stream takes."""
    import numpy as np
    n = min(max(int(valid), 0), 15)
    return {"fibs": [np.array(fib[j], np.uint8).reshape(3, 32) for j in range(15 - n, 15)],
            "crc_ok": [np.array(crc_ok[j], np.uint8).reshape(3) for j in range(15 - n, 15)], "next_count": int(next_count) & 0xFFFFFFFF}


def write_stream(streams, fibs, crc_ok, data, history=None, cif_start=None):
    """What one call on one ensemble stream must write.  fibs [n_cif][3][32] and crc_ok [n_cif][3] of this call's CIFs,
    data {stream id: [n_cif][bytes]} as the decoder aligns them (entry t belongs to CIF t - 15).  history: None or
    {"fibs": [...], "crc_ok": [...], "next_count": int} of the CIFs before this call (at most the last 15 are used).
    -> (frames, status [(cif_count, flags, fib_ok, length)], history for the next call)"""
    n_cif = len(fibs)
    old_f = list(history["fibs"])[-15:] if history else []
    old_k = list(history["crc_ok"])[-15:] if history else []
    anchor = next((c for c in range(n_cif) if fig0_0_count(fibs[c][0], crc_ok[c][0]) is not None), None)
    no_anchor = False
    if cif_start is not None and cif_start >= 0:
        base = cif_start % 5000
    elif anchor is not None:
        base = (fig0_0_count(fibs[anchor][0], 1) - anchor) % 5000
    else:
        no_anchor = True
        base = (int(history["next_count"]) & 0xFFFFFFFF) % 5000 if history and old_f else 0   # the record's int32 read as unsigned
    _, length = frame_length(streams)
    frames, status = [], []
    for t in range(n_cif):
        c = t - 15
        count = (base + c) % 5000
        if c >= 0:
            fic3, ok3 = fibs[c], crc_ok[c]
        elif -c <= len(old_f):
            fic3, ok3 = old_f[c], old_k[c]
        else:
            fic3, ok3 = None, None
        warm = fic3 is None
        flags = NO_ANCHOR if no_anchor else 0
        if warm:
            flags |= WARMUP
            fic, fib_ok = bytes(96), 0
        else:
            fic = b"".join(bytes(x) for x in fic3)
            fib_ok = sum(1 << j for j in range(3) if ok3[j])
            if fib_ok != 7:
                flags |= FIB_CRC
            own = fig0_0_count(fic3[0], ok3[0])
            if own is not None and own != count:
                flags |= COUNT_MISMATCH
        frames.append(write_frame(streams, count, fic, {i: d[t] for i, d in data.items()},
                                  err_byte([1, 1, 1] if warm else ok3, warm)))
        status.append((count, flags, fib_ok, length))
    hist = {"fibs": (old_f + [f for f in fibs])[-15:], "crc_ok": (old_k + [k for k in crc_ok])[-15:],
            "next_count": (base + n_cif) % 5000}
    return frames, status, hist
