"""The MOT directory carousel receiver from its definition: the contract at dabgpu_packet_carousel_dev in include/dabgpu.h
(EN 301 234 clause 7.2), read clause by clause into Python -- bytes, ints, dicts and lists, byte-serial, no shared code with
include/dabgpu_mot_carousel.h, the kernels or dabgpu/synth.py.  Where the contract says "word for word" of the packet call,
the frames and packets go through packet_reference.Receiver as that file stands (its scan, its steps a-g); the closed group
arrives here where it would arrive at mot_reference.Receiver._closed.

    rx = Receiver(directory_capacity, assemblies, object_capacity, address, fec)   # a fresh start; the state between calls
    objects, directory, counts = rx.call(frames, bitrate_kbps, max_objects, object_stride)
        objects: [(OBJECT_DTYPE record, header bytes, body bytes)] of this call; directory: the bytes d_directory received in
        this call, or None: every directory that became current, one written over the other from byte 0 (the last one wins;
        its length is in its own first four bytes; behind it may lie the end of a longer one before it); counts: a
        RESULT_DTYPE record
    parse_directory(bytes) -> (info dict, [object dicts]), None (mismatched) or "too_large"
"""
import numpy as np

import mot_reference as M
import packet_reference as P

COUNTERS = ("groups_header_mode", "groups_compressed_directory", "groups_unlisted", "directories_completed",
            "directories_mismatched", "directories_too_large", "objects_stale", "objects_evicted", "objects_dropped",
            "objects_deferred", "objects_written", "directory_id", "directory_bytes", "directory_objects", "directory_period",
            "directory_segment_size")
RESULT_DTYPE = np.dtype([("head", P.RESULT_DTYPE)] + [(n, np.int32) for n in COUNTERS])
OBJECT_DTYPE = np.dtype([(n, np.int32) for n in ("transport_id", "content_type", "content_subtype", "header_bytes", "body_bytes",
                                                  "frame", "slot", "directory_id")])
SEGMENTS, INDEX_MAX, GROUP_CAP = 256, 256, 16384


def arena_bytes(directory_capacity, assemblies, object_capacity):
    return GROUP_CAP + (directory_capacity + 15) // 16 * 16 + assemblies * ((object_capacity + 15) // 16 * 16)


def parse_directory(d):
    """the directory check, rules 1-7"""
    d = bytes(d)
    D = len(d)
    if D < 13 or int.from_bytes(d[0:4], "big") & 0x3FFFFFFF != D:                         # 1
        return None
    if d[0] & 0x80:                                                                       # 2
        return None
    N, period = int.from_bytes(d[4:6], "big"), int.from_bytes(d[6:9], "big")               # 3
    segment_size, X = int.from_bytes(d[9:11], "big") & 0x1FFF, int.from_bytes(d[11:13], "big")
    o = 13 + X
    if o > D:                                                                             # 4
        return None
    if N > INDEX_MAX:                                                                     # 5
        return "too_large"
    objects = []
    for _ in range(N):                                                                    # 6
        if o + 9 > D:
            return None
        tid, core = int.from_bytes(d[o:o + 2], "big"), int.from_bytes(d[o + 2:o + 9], "big")
        header_size = (core >> 15) & 0x1FFF
        if header_size < 7 or o + 2 + header_size > D:
            return None
        objects.append(dict(tid=tid, offset=o + 2, header_size=header_size, body_size=core >> 28, type=(core >> 9) & 0x3F,
                            subtype=core & 0x1FF))
        o += 2 + header_size
    if o != D:                                                                            # 7
        return None
    return dict(objects=N, period=period, segment_size=segment_size, extension_offset=13, extension_bytes=X, directory_bytes=D), objects


class Part:
    """a directory or a body under assembly"""

    def __init__(self, tid, cap, stamp=0):
        self.tid, self.cap, self.stamp = tid, cap, stamp
        self.size, self.last, self.last_len, self.segs, self.too_large = None, None, 0, {}, False

    def full(self):
        return self.last is not None and all(n in self.segs for n in range(self.last + 1))

    def data(self):
        """(the last segment counts with the length its last-segment group gave: it may have been placed earlier, as a longer
        segment that was not the last, and a segment present is not overwritten)"""
        return b"".join(self.segs[n] for n in range(self.last)) + self.segs[self.last][:self.last_len]

    def place(self, number, last, seg, n):
        """"Assembly" of dabgpu_mot_slides_dev from "n >= ..." on -> True when the segment was placed now"""
        z = len(seg)
        if number >= SEGMENTS:
            n["objects_too_large"] += 1
            self.too_large = True
            return False
        size = self.size
        if not last:
            if z == 0 or (size is not None and z != size) or (self.last is not None and number >= self.last):
                n["groups_malformed"] += 1
                return False
            size = z
        else:
            if number > 0 and size is None:
                n["segments_early_last"] += 1
                return False
            if (self.last is not None and (self.last != number or self.last_len != z)) or (size is not None and z > size) \
                    or any(m > number for m in self.segs):
                n["groups_malformed"] += 1
                return False
        at = number * (size or 0)
        if at + z > self.cap:
            n["objects_too_large"] += 1
            self.too_large = True
            return False
        if not last:
            self.size = size
        else:
            self.last, self.last_len = number, z
        if number in self.segs:
            n["segments_repeated"] += 1
            return False
        self.segs[number] = bytes(seg)
        n["segments_placed"] += 1
        n["object_bytes"] += z
        return True


class Carousel:
    """stands where packet_reference.Receiver keeps its mot_reference.Receiver: takes the closed groups"""

    def __init__(self, directory_capacity, assemblies, object_capacity):
        self.directory_capacity, self.K, self.object_capacity = directory_capacity, assemblies, object_capacity
        self.assembling = None             # the directory under assembly (a Part)
        self.current = None                # dict(tid, data, info, objects, delivered: set of index numbers)
        self.bodies = [None] * assemblies  # Parts
        self.placed = 0                    # body segments placed, mod 2^32
        self.n = dict.fromkeys(M.COUNTERS, 0)
        self.c = dict.fromkeys(COUNTERS, 0)
        self.where = (0, 0)
        self.objects, self.directory, self.deferred = [], None, set()
        self.max_objects, self.object_stride = 0, 0

    def _listed(self, tid):
        for i, e in enumerate(self.current["objects"]):
            if e["tid"] == tid:
                return i
        return None

    # -- closing a group
    def _closed(self, g):
        b0, end = g[0], len(g) - 2
        if not b0 & 0x40 or M.P.crc_ccitt(g[:end]) != (g[end] << 8 | g[end + 1]):
            self.n["groups_crc_failed"] += 1
            return
        dg_type = b0 & 0x0F
        if dg_type == 3:
            self.c["groups_header_mode"] += 1
            return
        if dg_type == 7:
            self.c["groups_compressed_directory"] += 1
            return
        if dg_type not in (4, 6):
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
        (self._directory_segment if dg_type == 6 else self._body_segment)(tid, number, bool(last), g[o:end])

    # -- the directory
    def _directory_segment(self, tid, number, last, seg):
        if self.current is not None and self.current["tid"] == tid:
            self.n["groups_repeated"] += 1
            return
        if self.current is not None or self.assembling is None or self.assembling.tid != tid:
            self.current = None
            self.assembling = Part(tid, self.directory_capacity)
        part = self.assembling
        if part.too_large:
            return
        part.place(number, last, seg, self.n)
        if part.full():
            self.assembling = None
            self._check(tid, part.data())

    def _check(self, tid, d):
        parsed = parse_directory(d)
        if parsed is None:
            self.c["directories_mismatched"] += 1
            return
        if parsed == "too_large":
            self.c["directories_too_large"] += 1
            return
        info, objects = parsed
        self.c["directories_completed"] += 1
        self.current = dict(tid=tid, data=d, info=info, objects=objects, delivered=set())
        self.directory = d + (self.directory or b"")[len(d):]
        self.n["object_bytes"] += len(d)
        for k, b in enumerate(self.bodies):
            if b is not None and self._listed(b.tid) is None:
                self.bodies[k] = None
                self.c["objects_stale"] += 1

    # -- bodies
    def _body_segment(self, tid, number, last, seg):
        if self.current is not None:
            i = self._listed(tid)
            if i is None:
                self.c["groups_unlisted"] += 1
                return
            if i in self.current["delivered"]:
                self.n["groups_repeated"] += 1
                return
        k = next((j for j, b in enumerate(self.bodies) if b is not None and b.tid == tid), None)
        if k is None:
            k = next((j for j, b in enumerate(self.bodies) if b is None), None)
            if k is None:
                ages = [(self.placed - b.stamp) % (1 << 32) for b in self.bodies]
                k = ages.index(max(ages))
                self.c["objects_evicted"] += 1
            self.bodies[k] = Part(tid, self.object_capacity, self.placed)
        b = self.bodies[k]
        if b.too_large:
            return
        if b.place(number, last, seg, self.n):
            self.placed = (self.placed + 1) % (1 << 32)
            b.stamp = self.placed

    # -- emission: one attempt behind every followed packet
    def attempt(self):
        if self.current is None:
            return
        for k, b in enumerate(self.bodies):
            if b is not None and b.full() and self._listed(b.tid) is not None:
                break
        else:
            return
        i = self._listed(b.tid)
        e, body = self.current["objects"][i], b.data()
        if len(body) != e["body_size"]:
            self.n["objects_mismatched"] += 1
            self.bodies[k] = None
            return
        if 32 + e["header_size"] + len(body) > self.object_stride:
            self.c["objects_dropped"] += 1
            self.current["delivered"].add(i)
            self.bodies[k] = None
            return
        if len(self.objects) >= self.max_objects:
            if k not in self.deferred:
                self.c["objects_deferred"] += 1
            self.deferred.add(k)
            return
        header = self.current["data"][e["offset"]:e["offset"] + e["header_size"]]
        rec = np.zeros(1, OBJECT_DTYPE)
        rec["transport_id"], rec["content_type"], rec["content_subtype"] = b.tid, e["type"], e["subtype"]
        rec["header_bytes"], rec["body_bytes"], rec["frame"], rec["slot"] = len(header), len(body), self.where[0], self.where[1]
        rec["directory_id"] = self.current["tid"]
        self.objects.append((rec, header, body))
        self.c["objects_written"] += 1
        self.n["objects_completed"] += 1
        self.n["object_bytes"] += len(header) + len(body)
        self.current["delivered"].add(i)
        self.bodies[k] = None


class Receiver(P.Receiver):
    def __init__(self, directory_capacity, assemblies, object_capacity, address, fec=0):
        super().__init__(object_capacity, address, fec)
        self.mot = Carousel(directory_capacity, assemblies, object_capacity)

    def _followed(self, k, pos, p, L):
        super()._followed(k, pos, p, L)
        self.mot.where = (k, pos)
        self.mot.attempt()

    def call(self, frames, bitrate_kbps, max_objects, object_stride):
        S = bitrate_kbps // 8
        self.n = dict.fromkeys(P.COUNTERS, 0)
        m = self.mot
        m.n, m.c = dict.fromkeys(M.COUNTERS, 0), dict.fromkeys(COUNTERS, 0)
        m.objects, m.directory, m.deferred, m.max_objects, m.object_stride = [], None, set(), max_objects, object_stride
        for k, frame in enumerate(frames):
            self._frame(k, bytes(np.asarray(frame, np.uint8)[:24 * S]), S)
        self.n["cifs"], self.n["slots"] = len(frames), len(frames) * S
        cur = m.current
        m.c["directory_id"] = cur["tid"] if cur else -1
        m.c["directory_bytes"] = len(cur["data"]) if cur else 0
        m.c["directory_objects"] = cur["info"]["objects"] if cur else 0
        m.c["directory_period"] = cur["info"]["period"] if cur else 0
        m.c["directory_segment_size"] = cur["info"]["segment_size"] if cur else 0
        rec = np.zeros(1, RESULT_DTYPE)
        for key in P.COUNTERS:
            rec["head"][key] = self.n[key]
        for key in M.COUNTERS:
            rec["head"]["mot"][key] = m.n[key]
        for key in COUNTERS:
            rec[key] = m.c[key]
        return m.objects, m.directory, rec


def delivered_so_far(results):
    return sum(int(r["objects_written"][0]) for r in results)
