"""The data-group receiver of any packet-mode component from its definition: the contract at dabgpu_packet_groups_dev in
include/dabgpu.h (EN 300 401 clauses 5.3.2, 5.3.3 and 6.3.6), read clause by clause into Python -- bytes, ints, dicts and lists,
byte-serial, no shared code with include/dabgpu_data_groups.h, the kernel or dabgpu/synth.py.  Frames and packets go through
packet_reference.Receiver as that file stands (its scan, its steps a-g); the closed group arrives here where it would arrive
at mot_reference.Receiver._closed.  Mode 1 restates steps a-c, which is all it has.

    rx = Receiver(address, fec, mode, keep_repeats)          # a fresh start; it is the state between calls
    out = rx.call(frames, bitrate_kbps, bytes_capacity, max_groups)
        out.groups: [(record dict, bytes)] emitted in this call (mode 1: break records, bytes b""); out.stream: mode 1, the
        emitted bytes; out.counts: dict of the result record; out.written: {offset: bytes} of d_bytes
    rx.state() -> dict(seen, prev, open, group bytes, last: {type: continuity})
    user_applications(fibs, crc_ok) -> [dict] sorted by (sid, scids, ua_type)
"""
import numpy as np

import packet_reference as P

EXTENSION, CRC, SEGMENT, USER_ACCESS, TRANSPORT_ID, REPEAT, BREAK = 1, 2, 4, 8, 16, 32, 64
COUNTERS = P.COUNTERS + ("groups_closed", "groups_malformed", "groups_crc_failed", "groups_no_crc", "groups_repeated",
                         "groups_emitted", "groups_no_room", "bytes_emitted", "bytes_no_room")
RECORD_FIELDS = ("offset", "length", "cif", "slot", "type", "continuity", "repetition", "flags", "extension", "segment",
                 "transport_id", "data_offset", "data_length")
OFFSET_SAT = 1 << 31


def parse_group(g):
    """clause 5.3.3.1 -> a record dict (without offset, cif, slot), "crc" or "malformed"; first match wins"""
    n = len(g)
    if n < 4:
        return "malformed"
    b0, b1 = g[0], g[1]
    has_crc = bool(b0 & 0x40)
    if has_crc and P.crc_bit_by_bit(g[:n - 2]) != (g[n - 2] << 8 | g[n - 1]):
        return "crc"
    end = n - 2 if has_crc else n
    o, flags, extension, segment, tid = 2, CRC if has_crc else 0, 0, -1, -1
    if b0 & 0x80:
        if o + 2 > end:
            return "malformed"
        extension, flags, o = g[o] << 8 | g[o + 1], flags | EXTENSION, o + 2
    if b0 & 0x20:
        if o + 2 > end:
            return "malformed"
        segment, flags, o = g[o] << 8 | g[o + 1], flags | SEGMENT, o + 2
    if b0 & 0x10:
        if o + 1 > end:
            return "malformed"
        ua = g[o]
        o += 1
        li, tid_flag = ua & 0x0F, bool(ua & 0x10)
        if (tid_flag and li < 2) or o + li > end:
            return "malformed"
        flags |= USER_ACCESS
        address_bytes = li
        if tid_flag:
            tid, flags, address_bytes = g[o] << 8 | g[o + 1], flags | TRANSPORT_ID, li - 2
        flags |= address_bytes << 8
        o += li
    return dict(length=n, type=b0 & 0x0F, continuity=b1 >> 4, repetition=b1 & 0x0F, flags=flags, extension=extension,
                segment=segment, transport_id=tid, data_offset=o, data_length=end - o)


class Result:
    def __init__(self):
        self.groups, self.stream, self.counts, self.written = [], b"", {}, {}


class Sink:
    """stands where packet_reference.Receiver keeps its mot_reference.Receiver: takes the closed groups of mode 0"""

    def __init__(self, keep_repeats):
        self.keep_repeats = keep_repeats
        self.last = {}                     # type -> continuity index of the latest accepted group
        self.where = (0, 0)
        self.start(0, 0)

    def start(self, bytes_capacity, max_groups):
        self.n = dict(groups_malformed=0)  # (packet_reference counts the groups below 4 bytes here)
        self.c = dict.fromkeys(COUNTERS, 0)
        self.cap, self.max_groups = bytes_capacity, max_groups
        self.index, self.offset = 0, 0
        self.out = Result()
        self.arrived = 0

    def _closed(self, g):
        self.arrived += 1
        r = parse_group(g)
        if r == "malformed":
            self.c["groups_malformed"] += 1
            return
        if r == "crc":
            self.c["groups_crc_failed"] += 1
            return
        if not r["flags"] & CRC:
            self.c["groups_no_crc"] += 1
        repeat = self.last.get(r["type"]) == r["continuity"]
        self.last[r["type"]] = r["continuity"]
        if repeat:
            self.c["groups_repeated"] += 1
            if not self.keep_repeats:
                return
            r["flags"] |= REPEAT
        i, offset = self.index, self.offset
        self.index += 1
        self.offset = min(offset + (len(g) + 15) // 16 * 16, OFFSET_SAT)
        if i < self.max_groups and offset + len(g) <= self.cap:
            r.update(offset=offset, cif=self.where[0], slot=self.where[1])
            self.out.groups.append((r, bytes(g)))
            self.out.written[offset] = bytes(g)
            self.c["groups_emitted"] += 1
            self.c["bytes_emitted"] += len(g)
        else:
            self.c["groups_no_room"] += 1


class Receiver(P.Receiver):
    def __init__(self, address, fec=0, mode=0, keep_repeats=0):
        super().__init__(0, address, fec)
        self.mode = mode
        self.mot = Sink(keep_repeats)

    # mode 1: steps a, b, c; nothing is ever open
    def _raw(self, k, pos, p, L):
        s = self.mot
        h0, h2 = p[0], p[2]
        ci, cmd, udl = (h0 >> 4) & 3, h2 >> 7, h2 & 0x7F
        if self.prev is not None and ci != (self.prev + 1) & 3:                       # a
            self.n["continuity_breaks"] += 1
            if s.index < s.max_groups:
                s.out.groups.append((dict(offset=s.offset, length=0, cif=k, slot=pos, type=0, continuity=0, repetition=0,
                                          flags=BREAK, extension=0, segment=0, transport_id=0, data_offset=0, data_length=0), b""))
                s.c["groups_emitted"] += 1
            else:
                s.c["groups_no_room"] += 1
            s.index += 1
        self.prev = ci
        if udl > 24 * L - 5:                                                          # b
            self.n["packets_malformed"] += 1
            return
        if cmd:                                                                       # c
            self.n["packets_command"] += 1
            return
        if s.offset + udl <= s.cap:
            s.out.written[s.offset] = bytes(p[3:3 + udl])
            s.out.stream += bytes(p[3:3 + udl])
            s.c["bytes_emitted"] += udl
        else:
            s.c["bytes_no_room"] += udl
        s.offset += udl

    def _followed(self, k, pos, p, L):
        if self.mode:
            self._raw(k, pos, p, L)
        else:
            super()._followed(k, pos, p, L)

    def call(self, frames, bitrate_kbps, bytes_capacity, max_groups):
        S = bitrate_kbps // 8
        self.n = dict.fromkeys(P.COUNTERS, 0)
        s = self.mot
        s.start(bytes_capacity, max_groups)
        if self.mode:
            self.group = None
        for k, frame in enumerate(frames):
            self._frame(k, bytes(np.asarray(frame, np.uint8)[:24 * S]), S)
        self.n["cifs"], self.n["slots"] = len(frames), len(frames) * S
        c = s.c
        for key in P.COUNTERS:
            c[key] = self.n[key]
        c["groups_malformed"] += s.n["groups_malformed"]
        c["groups_closed"] = s.arrived + s.n["groups_malformed"]
        s.out.counts = dict(c)
        return s.out

    def state(self):
        return dict(seen=self.prev is not None, prev=self.prev or 0, open=self.group is not None,
                    group=bytes(self.group) if self.group is not None else b"", last=dict(self.mot.last))


def total(results):
    return {k: sum(r.counts[k] for r in results) for k in COUNTERS}


# ---- FIG 0/13 and its joins (clauses 6.3.6, 6.3.5, 6.3.2) ---------------------------------------------------------------
def _figs(fibs, crc_ok):
    """the type-0 FIGs of the current configuration of this ensemble, in order: (extension, P/D, body bytes)"""
    fibs = np.asarray(fibs, np.uint8).reshape(-1, 32)
    for fib, ok in zip(fibs, np.asarray(crc_ok).reshape(-1)):
        if not ok:
            continue
        d, i = bytes(fib[:30]), 0
        while i < 30 and d[i] != 0xFF:
            kind, length = d[i] >> 5, d[i] & 0x1F
            if length == 0 or i + 1 + length > 30:
                break
            body = d[i + 1:i + 1 + length]
            i += 1 + length
            if kind == 0 and not body[0] & 0xC0:
                yield body[0] & 0x1F, (body[0] >> 5) & 1, body[1:]


def user_applications(fibs, crc_ok):
    figs = list(_figs(fibs, crc_ok))
    global_of, packet_of = {}, {}
    for ext, pd, b in figs:
        w = 4 if pd else 2
        if ext == 8:
            j = 0
            while j + w + 2 <= len(b):
                sid = int.from_bytes(b[j:j + w], "big")
                extended, scids, long_form = b[j + w] >> 7, b[j + w] & 0x0F, b[j + w + 1] >> 7
                j += w + 1
                size = (2 if long_form else 1) + extended
                if j + size > len(b):
                    break
                ident = int.from_bytes(b[j:j + 2], "big") & 0x0FFF if long_form else b[j] & 0x3F
                fidc = not long_form and b[j] & 0x40                  # MSC/FIC flag 1: not a sub-channel, passed over
                j += size
                if not fidc:
                    global_of.setdefault((sid, scids), (long_form, ident))
        elif ext == 3:
            j = 0
            while j + 5 <= len(b):
                scid, caorg = int.from_bytes(b[j:j + 2], "big") >> 4, b[j + 1] & 1
                entry = (b[j + 3] >> 2, int.from_bytes(b[j + 3:j + 5], "big") & 0x3FF)
                j += 5 + 2 * caorg
                if j > len(b):
                    break
                packet_of.setdefault(scid, entry)
    found = {}
    for ext, pd, b in figs:
        if ext != 13:
            continue
        w, j = 4 if pd else 2, 0
        while j + w + 1 <= len(b):
            sid = int.from_bytes(b[j:j + w], "big")
            scids, count = b[j + w] >> 4, b[j + w] & 0x0F
            j += w + 1
            cut = False
            for _ in range(count):
                if j + 2 > len(b):
                    cut = True
                    break
                word = int.from_bytes(b[j:j + 2], "big")
                ua_type, n = word >> 5, word & 0x1F
                if j + 2 + n > len(b):
                    cut = True
                    break
                data = bytes(b[j + 2:j + 2 + n])
                j += 2 + n
                if (sid, scids, ua_type) in found:
                    continue
                rec = dict(sid=sid, scids=scids, ua_type=ua_type, tmid_packet=0, subchid=-1, scid=-1, packet_address=-1, data=data)
                if (sid, scids) in global_of:
                    long_form, ident = global_of[(sid, scids)]
                    if not long_form:
                        rec["subchid"] = ident
                    else:
                        rec["tmid_packet"], rec["scid"] = 1, ident
                        if ident in packet_of:
                            rec["subchid"], rec["packet_address"] = packet_of[ident]
                found[(sid, scids, ua_type)] = rec
            if cut:
                break
    return [found[k] for k in sorted(found)]
