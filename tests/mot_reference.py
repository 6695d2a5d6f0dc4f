"""The slideshow receiver from its definition: the contract at dabgpu_mot_slides_dev in include/dabgpu.h (EN 300 401 clauses
5.3.3 and 7.4.5.1, EN 301 234 clauses 5.1, 5.2, 6.1, 6.2, TS 101 499 clause 6.2), read clause by clause into Python --
bytes, dicts and lists, no shared code with include/dabgpu_mot_walk.h.  The X-PAD field walk is the label reference's
(tests/pad_reference.py: locate_pad, split_field), as the contract says it is the label call's.

    rx = Receiver(body_capacity)          # a fresh start; it is the state (and the arena) between calls
    slides, counts = rx.call(data, status, n_superframes, s, max_slides, slide_stride)
        slides: [(MOT_SLIDE_DTYPE record, header bytes, body bytes)] of this call; counts: a RESULT_DTYPE record
    parse_header(header bytes) -> dict or None (refused)
"""
import numpy as np

import pad_reference as P

COUNTERS = ("aus", "aus_lost", "aus_with_xpad", "pad_malformed", "fields_ignored", "lengths_ok", "lengths_ignored", "groups_no_length",
            "groups_ok", "groups_crc_failed", "groups_ignored_type", "groups_no_transport_id", "groups_malformed", "groups_repeated",
            "segments_placed", "segments_repeated", "segments_early_last", "objects_completed", "objects_mismatched",
            "objects_too_large", "slides_written", "slides_dropped", "xpad_bytes", "object_bytes")
RESULT_DTYPE = np.dtype([(n, np.int32) for n in COUNTERS] + [("reserved", np.int32, (8,))])
SLIDE_DTYPE = np.dtype([(n, np.int32) for n in ("transport_id", "content_type", "content_subtype", "header_bytes", "body_bytes",
                                                 "superframe", "au", "reserved")])
HEADER_CAP, HEADER_SEGMENTS, BODY_SEGMENTS = 1024, 32, 256
ARENA_FIXED = 16384 + 1024


def arena_bytes(body_capacity):
    return ARENA_FIXED + (body_capacity + 15) // 16 * 16


class Part:
    def __init__(self, segments, cap):
        self.max_segments, self.cap = segments, cap
        self.size, self.last, self.segs = None, None, {}      # segment size, number of the last segment, number -> bytes

    def full(self):
        return self.last is not None and all(n in self.segs for n in range(self.last + 1))

    def data(self):
        return b"".join(self.segs[n] for n in range(self.last + 1))


class Receiver:
    def __init__(self, body_capacity):
        self.body_capacity = body_capacity
        self.cont, self.last_len = None, 0
        self.armed = None                  # the length a type-12 sub-field will consume
        self.group, self.need = None, 0    # the open data group
        self.tid, self.too_large, self.parts = None, False, None
        self.done = None                   # transport id of the object completed last
        self.n = dict.fromkeys(COUNTERS, 0)
        self.slides, self.where = [], (0, 0)

    # -- the object
    def _empty(self, tid):
        self.tid, self.too_large = tid, False
        self.parts = {3: Part(HEADER_SEGMENTS, HEADER_CAP), 4: Part(BODY_SEGMENTS, self.body_capacity)}

    def _segment(self, dg_type, tid, number, last, seg):
        if self.done is not None and tid == self.done:
            self.n["groups_repeated"] += 1
            return
        if self.tid is None or tid != self.tid:
            self._empty(tid)
        if self.too_large:
            return
        part, z = self.parts[dg_type], len(seg)
        if number >= part.max_segments:
            self.n["objects_too_large"] += 1
            self.too_large = True
            return
        size = part.size
        if not last:
            if z == 0 or (size is not None and z != size) or (part.last is not None and number >= part.last):
                self.n["groups_malformed"] += 1
                return
            size = z
        else:
            if number > 0 and size is None:
                self.n["segments_early_last"] += 1
                return
            if (part.last is not None and (part.last != number or len(part.segs[number]) != z)) or (size is not None and z > size) or any(m > number for m in part.segs):
                self.n["groups_malformed"] += 1
                return
        at = number * (size or 0)
        if at + z > part.cap:
            self.n["objects_too_large"] += 1
            self.too_large = True
            return
        if not last:
            part.size = size
        else:
            part.last = number
        if number in part.segs:
            self.n["segments_repeated"] += 1
        else:
            part.segs[number] = bytes(seg)
            self.n["segments_placed"] += 1
            self.n["object_bytes"] += z
        if self.parts[3].full() and self.parts[4].full():
            self._complete()

    def _complete(self):
        header, body, tid = self.parts[3].data(), self.parts[4].data(), self.tid
        self.tid, self.parts, self.too_large = None, None, False
        core = int.from_bytes(header[:7], "big") if len(header) >= 7 else None
        if core is None or (core >> 15) & 0x1FFF != len(header) or core >> 28 != len(body):
            self.n["objects_mismatched"] += 1
            return
        self.n["objects_completed"] += 1
        self.done = tid
        if len(self.slides) >= self.max_slides or 32 + len(header) + len(body) > self.slide_stride:
            self.n["slides_dropped"] += 1
            return
        rec = np.zeros(1, SLIDE_DTYPE)
        rec["transport_id"], rec["content_type"], rec["content_subtype"] = tid, (core >> 9) & 0x3F, core & 0x1FF
        rec["header_bytes"], rec["body_bytes"], rec["superframe"], rec["au"] = len(header), len(body), self.where[0], self.where[1]
        self.slides.append((rec, header, body))
        self.n["slides_written"] += 1
        self.n["object_bytes"] += len(header) + len(body)

    # -- data groups
    def _closed(self, g):
        b0, end = g[0], len(g) - 2
        if not b0 & 0x40 or P.crc_ccitt(g[:end]) != (g[end] << 8 | g[end + 1]):
            self.n["groups_crc_failed"] += 1
            return
        if b0 & 0x0F not in (3, 4):
            self.n["groups_ignored_type"] += 1
            return
        o = 4 if b0 & 0x80 else 2
        if not b0 & 0x20 or o + 2 > end:
            self.n["groups_malformed"] += 1
            return
        last, number = g[o] >> 7, (g[o] & 0x7F) << 8 | g[o + 1]
        o += 2
        if not b0 & 0x10:
            self.n["groups_no_transport_id"] += 1
            return
        if o + 1 > end:
            self.n["groups_malformed"] += 1
            return
        ua = g[o]
        o += 1
        if not ua & 0x10:
            self.n["groups_no_transport_id"] += 1
            return
        li = ua & 0x0F
        if li < 2 or o + li + 2 > end:
            self.n["groups_malformed"] += 1
            return
        tid = g[o] << 8 | g[o + 1]
        o += li
        z = (g[o] & 0x1F) << 8 | g[o + 1]
        o += 2
        if z != end - o:
            self.n["groups_malformed"] += 1
            return
        self.n["groups_ok"] += 1
        self._segment(b0 & 0x0F, tid, number, bool(last), g[o:end])

    def _subfield(self, typ, data):
        if typ == 1:
            if len(data) < 4 or P.crc_ccitt(data[:2]) != (data[2] << 8 | data[3]):
                self.n["lengths_ignored"] += 1
                return
            self.n["lengths_ok"] += 1
            self.armed = (data[0] & 0x3F) << 8 | data[1]
            return
        if typ == 12:
            self.group, armed, self.armed = None, self.armed, None
            if armed is None:
                self.n["groups_no_length"] += 1
                return
            if armed < 4:
                self.n["groups_malformed"] += 1
                return
            self.group, self.need = bytearray(), armed
        if typ in (12, 13) and self.group is not None:
            take = data[:self.need - len(self.group)]
            self.group += take
            self.n["xpad_bytes"] += len(take)
            if len(self.group) == self.need:
                g, self.group = bytes(self.group), None
                self._closed(g)

    # -- access units
    def _drop(self):
        self.cont, self.group, self.armed = None, None, None

    def access_unit(self, au):
        """au: bytes without the CRC, or None = lost"""
        self.n["aus"] += 1
        if au is None:
            self.n["aus_lost"] += 1
            self._drop()
            return
        pad = P.locate_pad(bytes(au))
        if pad is None:
            return
        field = "malformed" if pad == "malformed" else P.split_field(*pad, (self.cont, self.last_len))
        if field == "malformed":
            self.n["pad_malformed"] += 1
            self._drop()
            return
        if field == "ignored":
            self.n["fields_ignored"] += 1
            return
        subs, self.last_len = field
        if pad[1]:
            self.cont = None
        for typ, data in subs:
            self._subfield(typ, data)
            self.cont = P.continued_type(typ)
        if subs:
            self.n["aus_with_xpad"] += 1

    def call(self, data, status, n_superframes, s, max_slides, slide_stride):
        self.n = dict.fromkeys(COUNTERS, 0)
        self.slides, self.max_slides, self.slide_stride = [], max_slides, slide_stride
        status = np.asarray(status).view(P.STATUS_DTYPE).reshape(-1)
        for k in range(max(0, min(int(n_superframes), len(status)))):
            row, st = np.asarray(data[k], np.uint8), status[k]
            if not st["firecode_ok"] or st["num_aus"] <= 0:
                self.where = (k, 0)
                self.access_unit(None)
                continue
            for a in range(min(int(st["num_aus"]), 7)):
                b, e = int(st["au_start"][a]), int(st["au_start"][a + 1])
                good = (int(st["au_crc_mask"]) >> a) & 1 and 0 <= b and b + 2 < e <= 110 * s
                self.where = (k, a)
                self.access_unit(bytes(row[b:e - 2]) if good else None)
        rec = np.zeros(1, RESULT_DTYPE)
        for key in COUNTERS:
            rec[key] = self.n[key]
        return self.slides, rec


def total(results):
    return {k: sum(int(r[k][0]) for r in results) for k in COUNTERS}


# ---------------------------------------------------------------------------------------------- the MOT header
TEXT_PARAMS = {0x0C: "name", 0x26: "category_title", 0x27: "click_through_url", 0x28: "alternative_location_url"}


def parse_header(h):
    """-> what dabgpu.mot_header_parse returns, or None where it refuses with DABGPU_ERR_ARG, "capacity" with _CAPACITY"""
    h = bytes(h)
    if len(h) < 7:
        return None
    core = int.from_bytes(h[:7], "big")
    out = dict(body_size=core >> 28, header_size=(core >> 15) & 0x1FFF, content_type=(core >> 9) & 0x3F, content_subtype=core & 0x1FF,
               n_params=0, n_unknown=0, name=None, name_charset=None, trigger=None, expire=None, category_id=None, slide_id=None,
               category_title=None, click_through_url=None, alternative_location_url=None)
    if out["header_size"] != len(h):
        return None
    at = 7
    while at < len(h):
        pli, pid = h[at] >> 6, h[at] & 0x3F
        at += 1
        if pli < 3:
            n = (0, 1, 4)[pli]
        else:
            if at >= len(h):
                return None
            n = h[at] & 0x7F
            if h[at] & 0x80:
                if at + 1 >= len(h):
                    return None
                n = n << 8 | h[at + 1]
                at += 1
            at += 1
        if at + n > len(h):
            return None
        d = h[at:at + n]
        at += n
        out["n_params"] += 1
        if pid in TEXT_PARAMS:
            if pid == 0x0C:
                if not d:
                    return None
                out["name_charset"], d = d[0] >> 4, d[1:]
            if len(d) > 255:
                return "capacity"
            out[TEXT_PARAMS[pid]] = d
        elif pid in (0x05, 0x04):
            if n < 4:
                return None
            out["trigger" if pid == 0x05 else "expire"] = int.from_bytes(d[:4], "big") if d[0] >> 7 else "now"
        elif pid == 0x25:
            if n < 2:
                return None
            out["category_id"], out["slide_id"] = d[0], d[1]
        else:
            out["n_unknown"] += 1
    return out
