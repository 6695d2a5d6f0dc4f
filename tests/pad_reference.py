"""The dynamic-label receiver from its definition: the contract at dabgpu_pad_labels_dev in include/dabgpu.h (EN 300 401
clauses 7.4.2 - 7.4.5, TS 102 563 clause 5.4), read clause by clause into Python -- lists, bytes and dicts, no shared code
with include/dabgpu_pad_walk.h.  Works on what the follow call leaves: (data rows, status rows, n_superframes).

    st = Receiver()                       # a fresh start; it is the state between calls
    label, counts = st.call(data, status, n_superframes, s)      # PAD_LABEL_DTYPE / PAD_RESULT_DTYPE records of one call
    run_chunks(data, status, s, [5, 7])                           # one stream fed in calls of 5 and 7 super-frames
"""
import numpy as np

LABEL_DTYPE = np.dtype([("length", np.int32), ("charset", np.int32), ("toggle", np.int32), ("reserved", np.int32),
                        ("text", np.uint8, (128,))])
COUNTERS = ("aus", "aus_lost", "aus_with_xpad", "pad_malformed", "fields_ignored", "groups_ok", "groups_crc_failed",
            "commands_ignored", "labels_completed", "changes")
RESULT_DTYPE = np.dtype([(n, np.int32) for n in COUNTERS] + [("reserved", np.int32, (6,))])
STATUS_DTYPE = np.dtype([("firecode_ok", np.int32), ("rs_corrected", np.int32), ("rs_uncorrectable", np.int32),
                         ("num_aus", np.int32), ("au_crc_mask", np.int32), ("au_start", np.int32, (8,)),
                         ("reserved", np.int32, (3,))])
SUBFIELD_LENGTHS = (4, 6, 8, 12, 16, 24, 32, 48)


def crc_ccitt(data):
    """CCITT 0x1021, start 0xFFFF, complemented: as a division of the message polynomial, bit by bit"""
    reg = 0xFFFF
    for bit in np.unpackbits(np.frombuffer(bytes(data), np.uint8)).tolist():
        top = (reg >> 15) & 1
        reg = (reg << 1) & 0xFFFF
        if top ^ bit:
            reg ^= 0x1021
    return reg ^ 0xFFFF


def locate_pad(au):
    """au: the access unit without its CRC -> None (no PAD, or F-PAD says nothing changes), "malformed", or
    (ind, ci, the X-PAD's logical bytes)"""
    if len(au) < 2 or au[0] >> 5 != 4:
        return None
    n, o = au[1], 2
    if au[1] == 255:
        if len(au) == 2:                  # the escape byte itself is missing: o + n > len whatever it would have said
            return "malformed"
        n, o = n + au[2], 3
    if n < 2 or o + n > len(au):
        return "malformed"
    p = au[o:o + n]
    if p[n - 2] >> 6 != 0:
        return None
    ind, ci = (p[n - 2] >> 4) & 3, (p[n - 1] >> 1) & 1
    if ind in (0, 3):
        return None
    return ind, ci, bytes(p[:n - 2][::-1])


def split_field(ind, ci, x, context):
    """-> "malformed", "ignored" or the field's sub-fields [(type, bytes)] and the length the list leaves for a CI-less
    field behind it.  context = (continued type or None, that length)"""
    cont, last_len = context
    if ind == 1:
        if len(x) < 4:
            return "malformed"
        if ci:
            return [(x[0] & 0x1F, x[1:4])], 4
        if cont is None:
            return "ignored"
        return [(cont, x[0:4])], last_len
    if not ci:
        if cont is None:
            return "ignored"
        return [(cont, x[:min(last_len, len(x))])], last_len
    entries, at = [], 0
    while len(entries) < 4:
        if at >= len(x):
            return "malformed"
        length, typ = SUBFIELD_LENGTHS[x[at] >> 5], x[at] & 0x1F
        at += 1
        if typ == 0:
            break
        if typ == 31:
            if at >= len(x):
                return "malformed"
            at += 1
        entries.append((typ, length))
    if at + sum(length for _t, length in entries) > len(x):
        return "malformed"
    subs = []
    for typ, length in entries:
        subs.append((typ, x[at:at + length]))
        at += length
    return subs, (entries[-1][1] if entries else last_len)


def continued_type(typ):
    return 3 if typ in (2, 3) else 13 if typ in (12, 13) else None


class Receiver:
    """the state between calls: continuation context, open data group, segment assembly, current label"""

    def __init__(self):
        self.cont, self.last_len = None, 0
        self.group = None                  # bytearray of the open data group
        self.toggle, self.segments, self.last, self.charset = 0, {}, None, 0
        self.label = (0, 0, 0, b"")        # length, charset, toggle, text
        self.n = dict.fromkeys(COUNTERS, 0)

    # -- data groups
    def _needed(self, b0, b1):
        if not b0 & 0x10:
            return 2 + ((b0 & 0x0F) + 1) + 2
        if b0 & 0x0F == 1:
            return 4
        if b0 & 0x0F == 2:
            return 2 + ((b1 & 0x0F) + 1) + 2
        return None

    def _group_bytes(self, data):
        for v in data:
            if self.group is None:
                return
            self.group.append(v)
            if len(self.group) == 2 and self._needed(*self.group) is None:
                self.n["commands_ignored"] += 1
                self.group = None
            elif len(self.group) >= 2 and len(self.group) == self._needed(self.group[0], self.group[1]):
                g, self.group = bytes(self.group), None
                self._closed(g)

    def _closed(self, g):
        if crc_ccitt(g[:-2]) != (g[-2] << 8 | g[-1]):
            self.n["groups_crc_failed"] += 1
            return
        self.n["groups_ok"] += 1
        b0, b1 = g[0], g[1]
        if b0 & 0x10:
            if b0 & 0x0F == 1:
                self.segments, self.last, self.charset = {}, None, 0
                if self.label[0]:
                    self.n["changes"] += 1
                self.label = (0, 0, 0, b"")
            else:
                self.n["commands_ignored"] += 1
            return
        t, first, last = b0 >> 7, (b0 >> 6) & 1, (b0 >> 5) & 1
        if t != self.toggle:
            self.toggle, self.segments, self.last, self.charset = t, {}, None, 0
        number = 0 if first else (b1 >> 4) & 7
        if first:
            self.charset = b1 >> 4
        self.segments[number] = g[2:-2]
        if last:
            self.last = number
        if self.last is not None and all(m in self.segments for m in range(self.last + 1)):
            text = b"".join(self.segments[m] for m in range(self.last + 1))[:128]
            self.n["labels_completed"] += 1
            if (len(text), self.charset, text) != (self.label[0], self.label[1], self.label[3]):
                self.n["changes"] += 1
            self.label = (len(text), self.charset, self.toggle, text)
            self.segments, self.last, self.charset = {}, None, 0

    # -- access units
    def _drop(self):
        self.cont, self.group = None, None

    def access_unit(self, au):
        """au: bytes without the CRC, or None = lost"""
        self.n["aus"] += 1
        if au is None:
            self.n["aus_lost"] += 1
            self._drop()
            return
        pad = locate_pad(bytes(au))
        if pad is None:
            return
        field = "malformed" if pad == "malformed" else split_field(*pad, (self.cont, self.last_len))
        if field == "malformed":
            self.n["pad_malformed"] += 1
            self._drop()
            return
        if field == "ignored":
            self.n["fields_ignored"] += 1
            return
        subs, self.last_len = field
        if pad[1]:
            self.cont = None               # a list starts from no continued type
        for typ, data in subs:
            if typ == 2:
                self.group = bytearray()
            if typ in (2, 3):
                self._group_bytes(data)
            self.cont = continued_type(typ)
        if subs:
            self.n["aus_with_xpad"] += 1

    # -- calls
    def superframe(self, row, st, s):
        if not st["firecode_ok"] or st["num_aus"] <= 0:
            self.access_unit(None)
            return
        for a in range(min(int(st["num_aus"]), 7)):
            b, e = int(st["au_start"][a]), int(st["au_start"][a + 1])
            good = (int(st["au_crc_mask"]) >> a) & 1 and 0 <= b and b + 2 < e <= 110 * s
            self.access_unit(bytes(row[b:e - 2]) if good else None)

    def call(self, data, status, n_superframes, s):
        """-> (label record, result record of this call); rows beyond n_superframes are not looked at"""
        self.n = dict.fromkeys(COUNTERS, 0)
        status = np.asarray(status).view(STATUS_DTYPE).reshape(-1)
        n = max(0, min(int(n_superframes), len(status)))
        for k in range(n):
            self.superframe(np.asarray(data[k], np.uint8), status[k], s)
        return self.label_record(), self.result_record()

    def label_record(self):
        rec = np.zeros(1, LABEL_DTYPE)
        rec["length"], rec["charset"], rec["toggle"] = self.label[:3]
        rec["text"][0, :self.label[0]] = np.frombuffer(self.label[3], np.uint8)
        return rec

    def result_record(self):
        rec = np.zeros(1, RESULT_DTYPE)
        for k in COUNTERS:
            rec[k] = self.n[k]
        return rec


def run_chunks(data, status, s, chunks, receiver=None):
    """one stream of super-frames fed in calls of `chunks` super-frames each (0 allowed) -> [(label, result)] per call"""
    rx = receiver or Receiver()
    out, at = [], 0
    for n in chunks:
        out.append(rx.call(data[at:at + n], status[at:at + n], n, s))
        at += n
    return out


def total(results):
    """the summed counters of several calls' result records"""
    return {k: sum(int(r[k][0]) for r in results) for k in COUNTERS}
