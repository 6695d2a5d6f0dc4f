"""The packet-mode receiver from its definition: the contract at dabgpu_packet_slides_dev in include/dabgpu.h (EN 300 401
clauses 5.3.2 and 5.3.3), read clause by clause into Python -- bytes, ints and lists, byte-serial, no shared code with
include/dabgpu_packet_walk.h, the kernels or dabgpu/synth.py.  A closed data group goes to mot_reference.Receiver._closed as
that file stands: from there on it is the slideshow reference.

    rx = Receiver(body_capacity, address, fec)        # a fresh start; it is the state (and the arena) between calls
    slides, counts = rx.call(frames, bitrate_kbps, max_slides, slide_stride)
        frames: [n_cifs] rows of at least 3 * bitrate bytes; slides: [(SLIDE_DTYPE record, header bytes, body bytes)] of
        this call; counts: a RESULT_DTYPE record
"""
import numpy as np

import mot_reference as M

COUNTERS = ("cifs", "slots", "slots_bad", "packets_fec", "packets_padding", "packets_other", "packets_followed",
            "continuity_breaks", "packets_malformed", "packets_command", "packets_orphan", "groups_opened",
            "groups_unfinished", "groups_too_long", "group_bytes")
RESULT_DTYPE = np.dtype([(n, np.int32) for n in COUNTERS] + [("reserved", np.int32), ("mot", M.RESULT_DTYPE)])
GROUP_CAP = 16384


def _shift(reg, byte):
    """one byte into the register of x^16 + x^12 + x^5 + 1, bit by bit, most significant first"""
    for bit in range(7, -1, -1):
        top = (reg >> 15) & 1
        reg = (reg << 1) & 0xFFFF
        if top ^ ((byte >> bit) & 1):
            reg ^= 0x1021
    return reg


#: what a byte does to a register whose low byte is zero (the division is linear): the bit-by-bit definition, tabulated
_BY_BYTE = [_shift(0, b) for b in range(256)]


def crc(data):
    """register all ones, complemented; a byte at a time: reg' = (reg << 8) ^ _BY_BYTE[(reg >> 8) ^ byte]"""
    reg = 0xFFFF
    for byte in data:
        reg = ((reg << 8) & 0xFFFF) ^ _BY_BYTE[(reg >> 8) ^ byte]
    return reg ^ 0xFFFF


def crc_bit_by_bit(data):
    reg = 0xFFFF
    for byte in data:
        reg = _shift(reg, byte)
    return reg ^ 0xFFFF


class Receiver:
    def __init__(self, body_capacity, address, fec=0):
        self.mot = M.Receiver(body_capacity)
        self.address, self.fec = address, fec
        self.prev = None                   # continuity index of the followed packet before (None: none seen)
        self.group = None                  # the open data group
        self.n = dict.fromkeys(COUNTERS, 0)
        self.good_by_chance = 0            # (not part of the result: good packets the scan met where none was laid)

    def _drop(self):
        if self.group is not None:
            self.n["groups_unfinished"] += 1
        self.group = None

    def _followed(self, k, pos, p, L):
        h0, h2 = p[0], p[2]
        ci, first, last, cmd, udl = (h0 >> 4) & 3, (h0 >> 3) & 1, (h0 >> 2) & 1, h2 >> 7, h2 & 0x7F
        if self.prev is not None and ci != (self.prev + 1) & 3:                       # a
            self.n["continuity_breaks"] += 1
            self._drop()
        self.prev = ci
        if udl > 24 * L - 5:                                                          # b
            self.n["packets_malformed"] += 1
            self._drop()
            return
        if cmd:                                                                       # c
            self.n["packets_command"] += 1
            return
        if first:                                                                     # d
            self._drop()
            self.group = bytearray()
            self.n["groups_opened"] += 1
        elif self.group is None:
            self.n["packets_orphan"] += 1
            return
        if len(self.group) + udl > GROUP_CAP:                                         # e
            self.n["groups_too_long"] += 1
            self.group = None
            return
        self.group += p[3:3 + udl]                                                    # f
        self.n["group_bytes"] += udl
        if last:                                                                      # g
            g, self.group = bytes(self.group), None
            if len(g) < 4:
                self.mot.n["groups_malformed"] += 1
                return
            self.mot.where = (k, pos)
            self.mot._closed(g)

    def _frame(self, k, frame, S):
        pos = 0
        while pos < S:
            p = frame[24 * pos:]
            L, addr = (p[0] >> 6) + 1, (p[0] & 3) << 8 | p[1]
            if self.fec and addr == 1022 and L == 1:                                  # 1
                self.n["packets_fec"] += 1
                pos += 1
            elif pos + L > S:                                                         # 2
                self.n["slots_bad"] += 1
                pos += 1
            elif crc(p[:24 * L - 2]) != (p[24 * L - 2] << 8 | p[24 * L - 1]):         # 3
                self.n["slots_bad"] += 1
                pos += 1
            else:                                                                     # 4
                if addr == 0:
                    self.n["packets_padding"] += 1
                elif addr != self.address:
                    self.n["packets_other"] += 1
                else:
                    self.n["packets_followed"] += 1
                    self._followed(k, pos, p[:24 * L], L)
                pos += L

    def call(self, frames, bitrate_kbps, max_slides, slide_stride):
        S = bitrate_kbps // 8
        self.n = dict.fromkeys(COUNTERS, 0)
        m = self.mot
        m.n = dict.fromkeys(M.COUNTERS, 0)
        m.slides, m.max_slides, m.slide_stride = [], max_slides, slide_stride
        for k, frame in enumerate(frames):
            self._frame(k, bytes(np.asarray(frame, np.uint8)[:24 * S]), S)
        self.n["cifs"], self.n["slots"] = len(frames), len(frames) * S
        rec = np.zeros(1, RESULT_DTYPE)
        for key in COUNTERS:
            rec[key] = self.n[key]
        for key in M.COUNTERS:
            rec["mot"][key] = m.n[key]
        return m.slides, rec


def total(results):
    out = {k: sum(int(r[k][0]) for r in results) for k in COUNTERS}
    out.update({"mot." + k: sum(int(r["mot"][k][0]) for r in results) for k in M.COUNTERS})
    return out
