"""EDI packets from the definition (include/dabgpu_edi.h, the format stated as known): a writer and a parser in plain
Python, byte by byte, sharing nothing with the library, its header or its binding but synth.crc16.  What the ETI writer
decides -- the delay of 15 CIFs, the count, the ERR byte -- comes from tests/eti_reference.py.

All integers big-endian, bit fields MSB first:

    "AF" LEN(4) SEQ(2) AR(1) = 0x90 PT(1) = 'T' | TAG items: name(4) bits(4) value(ceil(bits / 8)) | CRC(2)

A stream is the dict of eti_reference: {id, start, bitrate, uep, eep_type, level}.
"""
import eti_reference as E
from dabgpu.synth import crc16

MAX_PACKET = 8192


class Malformed(ValueError):
    """header and CRC hold, the TAG items do not"""


class NotDeti(ValueError):
    """well formed, but not a DETI packet"""


class NotAPacket(ValueError):
    """header or CRC"""


def item(name, value, bits=None):
    name = name if isinstance(name, bytes) else name.encode("latin1")
    assert len(name) == 4
    bits = 8 * len(value) if bits is None else bits
    return name + bits.to_bytes(4, "big") + bytes(value)


def af_packet(payload, seq, ar=0x90, pt=b"T"):
    head = b"AF" + len(payload).to_bytes(4, "big") + (seq % 65536).to_bytes(2, "big") + bytes([ar]) + pt
    body = head + bytes(payload)
    return body + crc16(body).to_bytes(2, "big")


def deti_value(dlfc, stat, fic=None, mid=1, fp=None, mnsc=0xFFFF, time=None, rfud=None, rfa=0, rfu=0):
    """time: None or (utco, seconds, tsta); fic: None or 96 bytes; rfud: None or 3 bytes"""
    fcth, fct = divmod(dlfc, 250)
    fp = dlfc % 8 if fp is None else fp
    v = E._bits((1 if time else 0, 1), (1 if fic is not None else 0, 1), (1 if rfud else 0, 1), (fcth, 5), (fct, 8))
    v += E._bits((stat, 8), (mid, 2), (fp, 3), (rfa, 2), (rfu, 1), (mnsc, 16))
    if time:
        v += E._bits((time[0], 8), (time[1], 32), (time[2], 24))
    if fic is not None:
        assert len(fic) == 96
        v += bytes(fic)
    if rfud:
        assert len(rfud) == 3
        v += bytes(rfud)
    return v


def est_item(n, st, data):
    assert len(data) == 8 * E.stl_of(st)
    return item(b"est" + bytes([n]), E._bits((st["id"], 6), (st["start"], 10), (E.tpl_of(st), 6), (0, 2)) + bytes(data))


PTR_DETI = item("*ptr", b"DETI" + bytes(4))


def pad8(payload):
    return payload + bytes(-len(payload) % 8)


def packet_bytes(streams):
    return 10 + (126 + sum(11 + 8 * E.stl_of(st) for st in streams) + 7) // 8 * 8 + 2


def write_packet(streams, dlfc, seq, fic, data, stat, **deti):
    """The writer's packet: *ptr, deti, est1..estN by ascending start address, zero padding to 8 bytes.  data: {stream id:
    bytes of this CIF}"""
    payload = PTR_DETI + item("deti", deti_value(dlfc, stat, fic, **deti))
    for n, st in enumerate(E.ordered(streams), 1):
        payload += est_item(n, st, bytes(data[st["id"]]))
    p = af_packet(pad8(payload), seq)
    assert len(p) == packet_bytes(streams) or deti
    return p


def header(b, at=0):
    """H of the contract: the total length of a plausible packet at b[at:], else None"""
    h = b[at:at + 10]
    if len(h) < 10 or h[:2] != b"AF" or h[9:10] != b"T" or (h[8] & 0xF0) != 0x90:
        return None
    total = 12 + int.from_bytes(h[2:6], "big")
    return total if total <= MAX_PACKET else None


def items_of(payload):
    out, at = [], 0
    while len(payload) - at >= 8:
        name, bits = payload[at:at + 4], int.from_bytes(payload[at + 4:at + 8], "big")
        n = (bits + 7) // 8
        if at + 8 + n > len(payload):
            raise Malformed("item %r overruns" % name)
        out.append((name, bits, payload[at + 8:at + 8 + n], at + 8))
        at += 8 + n
    return out


def parse_payload(payload, base=10):
    """-> dict of a DETI packet's parts; Malformed or NotDeti"""
    detis, ests, foreign = [], {}, False
    twice = False
    for name, bits, v, at in items_of(payload):
        if name == b"*ptr":
            if bits != 64:
                raise Malformed("*ptr length")
            foreign |= v[:4] != b"DETI"
        elif name == b"deti":
            if bits < 16:
                raise Malformed("deti length")
            atstf, ficf, rfudf, fcth, fct = v[0] >> 7, (v[0] >> 6) & 1, (v[0] >> 5) & 1, v[0] & 31, v[1]
            if bits != 48 + 64 * atstf + 768 * ficf + 24 * rfudf or fcth > 19 or fct > 249:
                raise Malformed("deti")
            d = {"atstf": atstf, "ficf": ficf, "rfudf": rfudf, "dlfc": 250 * fcth + fct, "stat": v[2], "mid": v[3] >> 6,
                 "fp": (v[3] >> 3) & 7, "mnsc": int.from_bytes(v[4:6], "big"), "utco": 0, "seconds": 0, "tsta": 0xFFFFFF, "fic": None}
            w = 6
            if atstf:
                d["utco"], d["seconds"], d["tsta"] = v[6], int.from_bytes(v[7:11], "big"), int.from_bytes(v[11:14], "big")
                w = 14
            if ficf:
                d["fic"] = v[w:w + 96]
            detis.append(d)
        elif name[:3] == b"est" and 1 <= name[3] <= 64:
            if bits < 24 or (bits - 24) % 64 or (bits - 24) // 64 > 1023:
                raise Malformed("est length")
            if name[3] in ests:
                twice = True
                continue
            w = int.from_bytes(v[:3], "big")
            ests[name[3]] = {"scid": w >> 18, "sad": (w >> 8) & 0x3FF, "tpl": (w >> 2) & 0x3F, "stl": (bits - 24) // 64,
                             "data": v[3:], "at": base + at + 3}
    if len(detis) != 1 or foreign or twice or sorted(ests) != list(range(1, len(ests) + 1)):
        raise NotDeti()
    d = detis[0]
    d["streams"] = [ests[n] for n in range(1, len(ests) + 1)]
    return d


def read_packet(p):
    """Parse and check one whole packet -> dict; NotAPacket, Malformed or NotDeti"""
    p = bytes(p)
    if header(p) != len(p) or crc16(p[:-2]) != int.from_bytes(p[-2:], "big"):
        raise NotAPacket()
    d = parse_payload(p[10:-2])
    d["seq"], d["length"] = int.from_bytes(p[6:8], "big"), len(p)
    return d


def write_stream(streams, fibs, crc_ok, data, history=None, cif_start=None, seq_start=0):
    """What one call of the EDI writer on one ensemble must write: eti_reference.write_stream's decisions, every frame
    said again as a packet.  -> (the byte stream, status [(cif_count, flags, fib_ok, packet bytes)], history)"""
    frames, status, hist = E.write_stream(streams, fibs, crc_ok, data, history, cif_start)
    out = b""
    for t, (frame, st) in enumerate(zip(frames, status)):
        info = E.read_frame(frame)                      # the reference's own frame, read by the reference's own reader
        out += write_packet(streams, st[0], seq_start + t, info["fic"], {i: d[t] for i, d in data.items()}, info["err"])
    n = packet_bytes(streams)
    return out, [(c, f, k, n) for c, f, k, _ in status], hist
