"""dabgpu_packet_carousel_dev / dabgpu_packet_carousel_host (the objects of MOT directory carousels of packet-mode service
components) and dabgpu_mot_directory_parse, against tests/carousel_reference.py: object slots, records, d_directory and
counters byte for byte and count for count -- no tolerance anywhere -- every output between sentinel bytes.

The cases are streams of logical frames (STREAMS), each about one clause of the contract.  For every stream the named counts
are asserted on the REFERENCE's result first, so a stream is shown to be what its name says before the code under test is
held to it.  The CPU tests take each stream through dabgpu_packet_carousel_host, whole and cut into calls with state and
arena handed on; the GPU tests take all of them in one call, and the shapes only a device can get wrong.  The transmit side
is dabgpu/synth.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import carousel_reference as R
import packet_reference as PR
from conftest import ROOT
from test_device_asm import CSRC, kernel_metadata

ARG, CAPACITY = -1, -6
FILL, GAP = 0xA7, 64
ADDR = 7
NB = 256                                   # bytes of a result record


# ------------------------------------------------------------------------------------------------ building streams
def image(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def header(body_size, name=None, **kw):
    """a MOT header: the core alone (7 bytes) without a name"""
    return synth.mot_header(body_size, 2, 3, [synth.mot_param(synth.MOT_CONTENT_NAME, bytes([synth.CHARSET_UTF8 << 4]) + name)] if name is not None else [], **kw)


def objects(first_tid, sizes, seed, names=True):
    return [(first_tid + i, header(n, b"o%d" % i if names else None), image(n, seed + i)) for i, n in enumerate(sizes)]


def frames_of(bitrate, groups, sizes=(2,), address=ADDR):
    return synth.packet_frames(bitrate, [synth.packetise(groups, address, sizes)])


def directory_groups(tid, directory, seg=None):
    segs = synth.mot_segments(directory, seg or len(directory))
    return [synth.mot_group(6, tid, n, n == len(segs) - 1, s, continuity=n) for n, s in enumerate(segs)]


def flat(lists):
    return [g for groups in lists for g in groups]


def sent(objs, tids=None):
    return [(t, h, b) for t, h, b in objs if tids is None or t in tids]


def _streams():
    S = {}

    def add(name, groups, objs, bitrate=64, sizes=(2,), **kw):
        counts = kw.pop("counts")
        S[name] = dict(dict(bitrate=bitrate, frames=frames_of(bitrate, groups, sizes), objects=objs, counts=counts), **kw)

    # plain: a directory in 1 and in 3 segments, then three objects in order
    objs = objects(0x200, (100, 333, 47), 1)
    for nseg, dseg in ((1, None), (3, 20)):
        d, b = synth.mot_carousel_groups(0x10, objs, 120, dseg)
        assert len(d) == nseg
        add("plain, directory in %d" % nseg, d + flat(b), sent(objs),
            counts=dict(directories_completed=1, objects_written=3, groups_repeated=0, directory_id=0x10, directory_objects=3, segments_placed=nseg + 1 + 3 + 1))
    # out of order: bodies before their directory, emitted by consecutive packets in assembly order once the directory is
    # there; the directory's segments out of order, its last segment first
    d, b = synth.mot_carousel_groups(0x11, objs, 120, 20)
    assert len(d) == 3
    add("bodies first, directory out of order", flat(b) + [d[2], d[1], d[0], d[2]] + d, sent(objs), sizes=(4,),
        counts=dict(segments_early_last=1, directories_completed=1, objects_written=3, groups_repeated=3, groups_unlisted=0))
    # interleaved: four objects segment by segment
    objs4 = objects(0x300, (90, 100, 110, 95), 10)
    d, b = synth.mot_carousel_groups(0x12, objs4, 40)
    assert all(len(x) == 3 for x in b)
    inter = [b[i][n] for n in range(3) for i in range(4)]
    add("interleaved, K 4", d + inter, sent(objs4), assemblies=4, counts=dict(objects_written=4, objects_evicted=0))
    # K 2: a0 and b0 find empty assemblies, every later group of the first round evicts (10); the last segments x2 take an
    # assembly and are dropped (no size known: segments_early_last), so their assemblies keep the stamp they took: a2 takes 0,
    # b2 takes 1 (older), c2 and d2 both take 0 (a tie: the lowest), and b stays in 1.  Second round: a0 evicts 0, b0 finds b
    # in 1 (no eviction), the other ten evict: 10 + 10
    add("interleaved, K 2", d + inter + inter, [], assemblies=2, counts=dict(objects_written=0, objects_evicted=20, segments_early_last=6))
    # K 1: eleven evictions in the interleaved round; then object by object: a0 evicts d, and every completed object leaves
    # the assembly empty for the next
    add("interleaved, K 1", d + inter + flat(b), sent(objs4), assemblies=1, counts=dict(objects_written=4, objects_evicted=11 + 1))
    # a carousel repeated three times
    d, b = synth.mot_carousel_groups(0x13, objs, 120, 20)
    cycle = d + flat(b)
    add("three cycles", cycle * 3, sent(objs), counts=dict(groups_repeated=2 * len(cycle), directories_completed=1, objects_written=3))
    # the directory id changes in mid-cycle: one object kept, one stale
    a, b4, c3 = objects(0x400, (60,), 20)[0], objects(0x404, (150,), 21)[0], objects(0x403, (70,), 22)[0]
    two = objects(0x402, (130,), 23)[0]
    dA, bA = synth.mot_carousel_groups(0x20, [a, two, b4], 50)
    dB, bB = synth.mot_carousel_groups(0x21, [two, c3], 50)
    add("directory change", dA + bA[0] + bA[1][:1] + bA[2][:2] + dB + bB[0][1:] + bB[1] + bA[2], [a, two, c3],
        counts=dict(directories_completed=2, objects_stale=1, objects_written=3, groups_unlisted=len(bA[2]), directory_id=0x21))
    # directory sizes
    stray = synth.mot_group(4, 0x999, 0, True, b"stray")
    add("N 0", directory_groups(0x30, synth.mot_directory([])) + [stray], [], counts=dict(directories_completed=1, directory_objects=0, directory_bytes=13, groups_unlisted=1))
    one = objects(0x500, (30,), 30, names=False)
    assert len(one[0][1]) == 7
    d, b = synth.mot_carousel_groups(0x31, one, 64, period=1234, extension=b"\x01\x02\x03")
    add("N 1, header of 7", d + [stray] + flat(b), sent(one), counts=dict(objects_written=1, groups_unlisted=1, directory_period=1234, directory_bytes=13 + 3 + 9))
    many = [(0x1000 + i, header(10 + i % 3), None) for i in range(257)]
    body255 = image(10 + 255 % 3, 31)
    d256 = synth.mot_directory([(t, h) for t, h, _ in many[:256]])
    add("N 256", directory_groups(0x32, d256, 1000) + [synth.mot_group(4, 0x1000 + 255, 0, True, body255)], [(0x10FF, many[255][1], body255)], directory_capacity=4096,
        counts=dict(directories_completed=1, directory_objects=256, objects_written=1, directory_bytes=13 + 256 * 9))
    d257 = synth.mot_directory([(t, h) for t, h, _ in many])
    add("N 257", directory_groups(0x33, d257, 1000) + [stray], [], directory_capacity=4096, counts=dict(directories_too_large=1, directories_completed=0, groups_unlisted=0, directory_id=-1))
    twice = synth.mot_directory([(0x600, header(50, b"first")), (0x601, header(20, b"between")), (0x600, header(60, b"second"))])
    b50 = image(50, 32)
    g50 = synth.mot_group(4, 0x600, 0, True, b50)
    add("duplicate transport id", directory_groups(0x34, twice) + [g50, g50, stray], [(0x600, header(50, b"first"), b50)],
        counts=dict(objects_written=1, groups_repeated=1, groups_unlisted=1, directory_objects=3))
    # the directory check, each rule once
    good = [(0x700, header(25, b"a")), (0x701, header(26, b"bb"))]
    dgood = synth.mot_directory(good)
    beyond = bytearray(dgood)
    beyond[11:13] = (len(dgood) - 12).to_bytes(2, "big")
    bad = {"wrong DirectorySize": synth.mot_directory(good, size=len(dgood) + 1),
           "compression bit": synth.mot_directory(good, compressed=True),
           "X beyond D": bytes(beyond),
           "header_size 6": synth.mot_directory([good[0], (0x701, synth.mot_header(26, 2, 3, header_size=6))]),
           "entry past D": synth.mot_directory([good[0], (0x701, header(26, b"bb", header_size=30))]),
           "trailing bytes": synth.mot_directory(good + [(0x702, header(5))], count=2)}
    for name, d in bad.items():
        add("check: " + name, directory_groups(0x35, d, 16) + [stray], [], counts=dict(directories_mismatched=1, directories_completed=0, groups_unlisted=0, segments_placed=-(-len(d) // 16) + 1))
    # other data group types, and types 4 / 6 with a failed or absent group CRC
    def broken(g):
        return g[:-1] + bytes([g[-1] ^ 1])
    d, b = synth.mot_carousel_groups(0x36, one, 64)
    others = [synth.mot_group(3, 0x500, 0, True, one[0][1]), synth.mot_group(7, 0x36, 0, True, b"compressed"), synth.msc_data_group(5, b"ca"),
              broken(d[0]), broken(b[0][0]), synth.mot_group(6, 0x36, 0, True, dgood, crc=False), synth.mot_group(4, 0x500, 0, True, b"nocrc", crc=False)]
    add("other types", others + d + flat(b), sent(one),
        counts=dict(groups_header_mode=1, groups_compressed_directory=1, groups_ignored_type=1, groups_crc_failed=4, objects_written=1))
    # caps
    objs = objects(0x800, (64,), 40)
    d, b = synth.mot_carousel_groups(0x37, objs, 30, 10)
    D = 13 + 2 + len(objs[0][1])
    add("directory of exactly directory_capacity", d + flat(b), sent(objs), directory_capacity=D, counts=dict(directories_completed=1, objects_written=1, directory_bytes=D))
    add("directory one byte more", d + flat(b) + d, [], directory_capacity=D - 1, counts=dict(directories_completed=0, objects_too_large=1, objects_written=0))
    add("body of exactly object_capacity", d + flat(b), sent(objs), object_capacity=64, counts=dict(objects_written=1, objects_too_large=0))
    add("body one byte more", d + flat(b) + flat(b), [], object_capacity=63, counts=dict(objects_written=0, objects_too_large=1))
    objs = objects(0x810, (257,), 41)
    d, b = synth.mot_carousel_groups(0x38, objs, 1)
    add("segment 256", d + flat(b), [], sizes=(1,), counts=dict(objects_too_large=1, segments_placed=1 + 256, objects_written=0))
    # a part that becomes full by a repetition: segment 0 placed as a non-last segment, then sent again as the last one, shorter
    # and with other bytes: the part's length is what the last-segment group said, its bytes are those placed first
    small = synth.mot_directory([(0x820, header(5))])
    first = synth.mot_group(6, 0x3F, 0, False, small + b"behind the directory")
    again = synth.mot_group(6, 0x3F, 0, True, bytes(len(small)))
    b8 = image(8, 42)
    add("a repetition completes the part", [first, again, synth.mot_group(4, 0x820, 0, False, b8), synth.mot_group(4, 0x820, 0, True, bytes(5))],
        [(0x820, header(5), b8[:5])], counts=dict(segments_placed=2, segments_repeated=2, directories_completed=1, directory_bytes=len(small), objects_written=1))
    # emission
    objs = objects(0x900, (80, 81, 82), 50)
    d, b = synth.mot_carousel_groups(0x39, [(objs[0][0], header(79, b"o0"), objs[0][2])] + objs[1:], 50)
    add("body_size mismatch", d + flat(b), sent(objs[1:]), counts=dict(objects_mismatched=1, objects_written=2))
    big = objects(0x910, (80, 120, 130), 53)
    d, b = synth.mot_carousel_groups(0x3A, big, 50)
    fits = 32 + len(big[0][1]) + 80
    add("an object too large for its slot", d + flat(b) + b[1], sent(big[:1]), object_stride=(fits + 15) // 16 * 16,
        counts=dict(objects_dropped=2, objects_written=1, groups_repeated=len(b[1])))
    d, b = synth.mot_carousel_groups(0x3A, objs, 50)
    add("more objects than slots", d + flat(b) + d, sent(objs[:1]), max_objects=1, cut_visible=True,
        counts=dict(objects_written=1, objects_deferred=1, groups_repeated=len(d)))
    # sizes where only device code can err
    segs = (1, 15, 16, 17, 63, 64, 65, 8191)
    objs = [(0xA00 + i, header(2 * s + s // 2 + 1, b"s%d" % s), image(2 * s + s // 2 + 1, 60 + i)) for i, s in enumerate(segs)]
    dd = synth.mot_directory([(t, h) for t, h, _ in objs])
    groups = directory_groups(0x3B, dd, 17)
    for (t, h, body), s in zip(objs, segs):
        pieces = synth.mot_segments(body, s)
        groups += [synth.mot_group(4, t, n, n == len(pieces) - 1, p) for n, p in enumerate(pieces)]
    add("segment sizes", groups, sent(objs), bitrate=512, sizes=(4, 1, 3), object_capacity=3 * 8191, object_stride=3 * 8192 + 64, max_objects=8,
        counts=dict(objects_written=8, directories_completed=1))
    objs = [(0xB00 + i, header(20 + i, b"n%04d" % i), image(20 + i, 70 + i)) for i in range(17)]    # (entries of 17 bytes)
    d, b = synth.mot_carousel_groups(0x3C, objs, 11, 33)
    offsets = {o["offset"] % 16 for o in R.parse_directory(synth.mot_directory([(t, h) for t, h, _ in objs]))[1]}
    assert offsets == set(range(16))
    add("header offsets of every residue", d + flat(b), sent(objs), bitrate=72, sizes=(3, 1), max_objects=17, object_stride=128, counts=dict(objects_written=17))
    objs = objects(0xC00, (66000,), 80)
    d, b = synth.mot_carousel_groups(0x3D, objs, 1000)
    add("a body of more than 64 KiB", d + flat(b), sent(objs), bitrate=512, sizes=(4,), object_capacity=66000, object_stride=66000 + 64,
        counts=dict(objects_written=1, segments_placed=1 + 66, object_bytes=len(synth.mot_directory([(objs[0][0], objs[0][1])])) * 2 + 2 * 66000 + len(objs[0][1])))
    objs = objects(0xD00, (10,), 81, names=False)
    d, b = synth.mot_carousel_groups(0x3E, objs, 10)
    add("rate 8", d + flat(b), sent(objs), bitrate=8, sizes=(1,), counts=dict(objects_written=1, slots=len(frames_of(8, d + flat(b), (1,)))))
    # three addresses on one d_in, at 72 kbit/s
    per = []
    for i, address in enumerate((ADDR, 8, 9)):
        objs = objects(0xE00 + 16 * i, (40 + i, 90 + i), 90 + 2 * i)
        d, b = synth.mot_carousel_groups(0x40 + i, objs, 32)
        per.append((address, synth.packetise(d + flat(b), address, (2, 1)), objs))
    shared = synth.packet_frames(72, [p for _a, p, _o in per])
    for address, pk, objs in per:
        S["shared, address %d" % address] = dict(bitrate=72, frames=shared, address=address, objects=sent(objs), share="shared, address %d" % ADDR,
                                                  counts=dict(objects_written=2, packets_followed=len(pk), packets_other=sum(len(q) for a, q, _o in per if a != address)))
    assert all(len(st["frames"]) <= 68 for st in S.values()), {k: len(v["frames"]) for k, v in S.items()}
    return S


_STREAMS = {}


def streams():
    if not _STREAMS:
        _STREAMS.update(_streams())
    return _STREAMS


STREAM_NAMES = (["plain, directory in 1", "plain, directory in 3", "bodies first, directory out of order", "interleaved, K 4", "interleaved, K 2",
                 "interleaved, K 1", "three cycles", "directory change", "N 0", "N 1, header of 7", "N 256", "N 257", "duplicate transport id"] +
                ["check: " + n for n in ("wrong DirectorySize", "compression bit", "X beyond D", "header_size 6", "entry past D", "trailing bytes")] +
                ["other types", "directory of exactly directory_capacity", "directory one byte more", "body of exactly object_capacity", "body one byte more",
                 "segment 256", "a repetition completes the part", "body_size mismatch", "an object too large for its slot", "more objects than slots", "segment sizes",
                 "header offsets of every residue", "a body of more than 64 KiB", "rate 8", "shared, address 7", "shared, address 8", "shared, address 9"])


# ------------------------------------------------------------------------------------------------ running a call
class HostMemory:
    def load(self, img):
        raw = np.empty(img.size + 256, np.uint8)
        off = -raw.ctypes.data % 256
        self.buf = raw[off:off + img.size]
        self.buf[:] = img
        return self.buf.ctypes.data

    def run(self, entries, n_cifs):
        dabgpu.packet_carousel_host(entries, n_cifs)

    def read(self):
        return self.buf.copy()


class DeviceMemory:
    def __init__(self, ctx):
        self.ctx = ctx

    def load(self, img):
        import torch
        self.t = torch.from_numpy(img).cuda()
        return self.t.data_ptr()

    def run(self, entries, n_cifs):
        self.ctx.packet_carousel_dev(entries, n_cifs)
        self.ctx.sync()

    def read(self):
        self.ctx.sync()
        return self.t.cpu().numpy()


DEFAULTS = dict(address=ADDR, fec=0, directory_capacity=1024, assemblies=4, object_capacity=512, max_objects=4, object_stride=1024)
KEYS = ("bitrate", "frames", "stride", "in_off", "state", "arena") + tuple(DEFAULTS)


def spec_of(st, a=0, b=None, **kw):
    sp = dict(DEFAULTS)
    sp.update({k: v for k, v in st.items() if k in KEYS})
    sp["frames"] = st["frames"][a:b]
    sp.update(kw)
    return sp


def sizes_of(sp):
    return sp["directory_capacity"], sp["assemblies"], sp["object_capacity"]


def call(mem, specs, n_cifs, mutate=None, refused=None, shared=()):
    """One call on buffers laid out in one allocation, every region between sentinel bytes.  specs: dicts of spec_of();
    shared: {entry: the entry whose frames it names}.  After the call nothing but state-out, arena, result, the written bytes
    of the slots and of d_directory may have changed (nothing at all for a refused call).  -> per entry dict(objects
    [(record, header, body)], directory (bytes or None), result, state, arena)"""
    size, lay = 0, []

    def take(n):
        nonlocal size
        off = (size + GAP + 255) // 256 * 256
        size = off + n
        return off

    nb = dabgpu.packet_carousel_state_bytes()
    for e, sp in enumerate(specs):
        stride = sp.get("stride", 3 * sp["bitrate"])
        ab = dabgpu.packet_carousel_arena_bytes(*sizes_of(sp))
        assert ab == R.arena_bytes(*sizes_of(sp))
        frames = lay[shared[e]]["frames"] if e in shared else take(max(n_cifs, 1) * stride + 16) + sp.get("in_off", 0)
        lay.append(dict(frames=frames, sin=take(nb) if sp.get("state") is not None else None, sout=take(nb), arena=take(ab), ab=ab,
                        objects=take(max(sp["max_objects"], 1) * sp["object_stride"]), directory=take(sp["directory_capacity"]), result=take(NB)))
    img = np.full(size + GAP, FILL, np.uint8)
    for e, (sp, L) in enumerate(zip(specs, lay)):
        stride = sp.get("stride", 3 * sp["bitrate"])
        if e not in shared:
            for k in range(n_cifs):
                img[L["frames"] + k * stride:L["frames"] + k * stride + 3 * sp["bitrate"]] = sp["frames"][k]
        if L["sin"] is not None:
            img[L["sin"]:L["sin"] + nb] = np.frombuffer(bytes(sp["state"]), np.uint8)
        if sp.get("arena") is not None:
            img[L["arena"]:L["arena"] + L["ab"]] = sp["arena"]
    base = mem.load(img)
    assert base % 256 == 0
    entries = [dabgpu.PacketCarouselEntry(base + L["frames"], sp.get("stride", 3 * sp["bitrate"]), sp["bitrate"], sp["address"], sp["fec"], sp["assemblies"],
                                          base + L["sin"] if L["sin"] is not None else None, base + L["sout"], base + L["arena"], L["ab"],
                                          base + L["objects"], sp["object_stride"], sp["max_objects"], sp["object_capacity"],
                                          base + L["directory"], sp["directory_capacity"], 0, base + L["result"]) for sp, L in zip(specs, lay)]
    if mutate:
        mutate(entries)
    if refused is not None:
        with pytest.raises(dabgpu.DabGpuError) as err:
            mem.run(entries, n_cifs)
        assert err.value.status == refused
        assert (mem.read() == img).all(), "a refused call wrote"
        return None
    mem.run(entries, n_cifs)
    after = mem.read()
    out, untouched = [], np.ones(after.size, bool)
    for sp, L in zip(specs, lay):
        for key, n in (("sout", nb), ("arena", L["ab"]), ("result", NB)):
            untouched[L[key]:L[key] + n] = False
        res = after[L["result"]:L["result"] + NB].copy().view(dabgpu.PACKET_CAROUSEL_RESULT_DTYPE)
        written = int(res["objects_written"][0])
        assert 0 <= written <= sp["max_objects"]
        objs = []
        for k in range(written):
            at = L["objects"] + k * sp["object_stride"]
            rec = after[at:at + 32].copy().view(dabgpu.MOT_CAROUSEL_OBJECT_DTYPE)
            hb, bb = int(rec["header_bytes"][0]), int(rec["body_bytes"][0])
            assert 0 <= hb and 0 <= bb and 32 + hb + bb <= sp["object_stride"], rec
            untouched[at:at + 32 + hb + bb] = False
            objs.append((rec, after[at + 32:at + 32 + hb].tobytes(), after[at + 32 + hb:at + 32 + hb + bb].tobytes()))
        # (d_directory: same() holds the whole buffer to what the reference says it received)
        untouched[L["directory"]:L["directory"] + sp["directory_capacity"]] = False
        directory = after[L["directory"]:L["directory"] + sp["directory_capacity"]].tobytes()
        out.append(dict(objects=objs, directory=directory, result=res, state=after[L["sout"]:L["sout"] + nb].copy(),
                        arena=after[L["arena"]:L["arena"] + L["ab"]].copy()))
    assert (after[untouched] == img[untouched]).all(), "bytes outside the outputs changed"
    return out


def same(got, want):
    """got: an entry of call(); want: (objects, directory, result record) of the reference: byte for byte"""
    wo, wd, wr = want
    wd = wd or b""
    return (got["result"].tobytes() == wr.tobytes() and got["directory"] == wd + bytes([FILL]) * (len(got["directory"]) - len(wd)) and
            len(got["objects"]) == len(wo) and
            all(g[0].tobytes() == w[0].tobytes() and g[1] == w[1] and g[2] == w[2] for g, w in zip(got["objects"], wo)))


def explain(got, want):
    return "\n got  %s %s\n want %s %s" % ([g[0] for g in got["objects"]], got["result"], [w[0] for w in want[0]], want[2])


def receiver(sp):
    return R.Receiver(*sizes_of(sp), sp["address"], sp["fec"])


def ref_call(rx, sp, a=0, b=None):
    return rx.call(sp["frames"][a:b], sp["bitrate"], sp["max_objects"], sp["object_stride"])


_WANTS = {}


def wanted(name):
    """the reference's answer to a whole stream: computed once, shared, left as it is"""
    if name not in _WANTS:
        sp = spec_of(streams()[name])
        _WANTS[name] = ref_call(receiver(sp), sp)
    return _WANTS[name]


def count_of(rec, key):
    if key in R.COUNTERS:
        return int(rec[key][0])
    return int((rec["head"][key] if key in PR.COUNTERS else rec["head"]["mot"][key])[0])


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_records_and_sizes(built, tmp_path):
    L = dabgpu.lib()
    for name in ("dabgpu_packet_carousel_state_bytes", "dabgpu_packet_carousel_arena_bytes", "dabgpu_packet_carousel_dev", "dabgpu_packet_carousel_host",
                 "dabgpu_mot_directory_parse"):
        assert name in dabgpu.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert dabgpu.PACKET_CAROUSEL_RESULT_DTYPE.itemsize == NB == R.RESULT_DTYPE.itemsize and dabgpu.PACKET_CAROUSEL_RESULT_DTYPE.names == R.RESULT_DTYPE.names
    assert dabgpu.MOT_CAROUSEL_OBJECT_DTYPE == R.OBJECT_DTYPE and hasattr(dabgpu.Context, "packet_carousel_dev")
    assert dabgpu.packet_carousel_state_bytes() % 16 == 0 and dabgpu.packet_carousel_state_bytes() > dabgpu.packet_state_bytes() + 32 * 48 + 256 * 12
    for sizes in ((16, 1, 0), (17, 3, 1), (1 << 20, 32, 256 * 8191), (1000, 7, 12345)):
        assert dabgpu.packet_carousel_arena_bytes(*sizes) == R.arena_bytes(*sizes)
    for sizes in ((15, 1, 0), ((1 << 20) + 1, 1, 0), (16, 0, 0), (16, 33, 0), (16, 1, -1), (16, 1, 256 * 8191 + 1)):
        assert L.dabgpu_packet_carousel_arena_bytes(*sizes) == 0
    # the binding's structures and the records against the header, as the C compiler lays them out
    structs = [("dabgpu_packet_carousel_entry", dabgpu.PacketCarouselEntry)]
    records = [("dabgpu_packet_carousel_result", dabgpu.PACKET_CAROUSEL_RESULT_DTYPE), ("dabgpu_mot_carousel_object", dabgpu.MOT_CAROUSEL_OBJECT_DTYPE),
               ("dabgpu_mot_directory", dabgpu.MOT_DIRECTORY_DTYPE), ("dabgpu_mot_directory_object", dabgpu.MOT_DIRECTORY_OBJECT_DTYPE)]
    lines, want = ['#include <stdio.h>', '#include <stddef.h>', '#include "dabgpu.h"', 'int main(void) {'], []
    for cname, cls in structs:
        lines.append('  printf(" %%zu", sizeof(%s));' % cname)
        lines += ['  printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f, _ in cls._fields_]
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    for cname, dt in records:
        lines.append('  printf(" %%zu", sizeof(%s));' % cname)
        lines += ['  printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f in dt.names]
        want += [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ['  return 0; }']) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == want


def test_transmit_side_is_what_the_standard_says():
    """one small directory, byte by byte from EN 301 234 clause 7.2.2, and the groups of its carousel"""
    h1, h2 = synth.mot_header(5, 2, 1), synth.mot_header(300, 2, 3, [synth.mot_param(synth.MOT_CONTENT_NAME, b"\xf0" + b"ab")])
    assert h1 == bytes([0x00, 0x00, 0x00, 0x50, 0x03, 0x84, 0x01])     # body 5 << 28 | header 7 << 15 | type 2 << 9 | subtype 1
    want = (bytes([0x00, 0x00, 0x00, 13 + 2 + (2 + 7) + (2 + len(h2))])  # CompressionFlag 0, Rfu 0, DirectorySize
            + bytes([0x00, 0x02])                                     # NumberOfObjects
            + bytes([0x00, 0x02, 0x58])                               # CarouselPeriod: 600 tenths of a second
            + bytes([0x00, 0x80])                                     # Rfu, Rfa, SegmentSize 128
            + bytes([0x00, 0x02]) + b"\xaa\xbb"                       # DirectoryExtensionLength, DirectoryExtension
            + bytes([0x12, 0x34]) + h1 + bytes([0xab, 0xcd]) + h2)    # TransportId, MOT header; twice
    d = synth.mot_directory([(0x1234, h1), (0xABCD, h2)], period=600, segment_size=128, extension=b"\xaa\xbb")
    assert d == want and len(d) == want[3]
    assert synth.mot_directory([], compressed=True)[0] == 0x80 and synth.mot_directory([], size=77)[:4] == bytes([0, 0, 0, 77])
    dg, bodies = synth.mot_carousel_groups(0x77, [(0x1234, h1, b"hello"), (0xABCD, h2, bytes(300))], 128, 16)
    assert [g[0] & 0x0F for g in dg] == [6] * len(dg) and len(dg) == -(-len(synth.mot_directory([(0x1234, h1), (0xABCD, h2)])) // 16)
    assert [[g[0] & 0x0F for g in b] for b in bodies] == [[4], [4, 4, 4]]
    # a type-6 group: CRC, segment and user access flags; segment number with the last flag; transport id; segmentation header
    last = dg[-1]
    assert last[0] == 0x76 and int.from_bytes(last[2:4], "big") == 0x8000 | (len(dg) - 1) and last[4] == 0x12 and last[5:7] == bytes([0x00, 0x77])
    assert int.from_bytes(last[7:9], "big") & 0x1FFF == len(last) - 9 - 2
    assert b"".join(g[9:-2] for g in dg) == synth.mot_directory([(0x1234, h1), (0xABCD, h2)])


def test_directory_parse_equals_the_reference(built):
    seen = 0
    for name in STREAM_NAMES:
        d = wanted(name)[1]
        if d is None:
            continue
        d = d[:int.from_bytes(d[:4], "big") & 0x3FFFFFFF]            # (the last one; the end of a longer one may lie behind it)
        info, objs = dabgpu.mot_directory_parse(d)
        winfo, wobjs = R.parse_directory(d)
        assert {k: int(info[k]) for k in winfo} == winfo, name
        assert [(int(o["transport_id"]), int(o["header_offset"]), int(o["header_bytes"]), int(o["body_bytes"]), int(o["content_type"]), int(o["content_subtype"])) for o in objs] == \
            [(o["tid"], o["offset"], o["header_size"], o["body_size"], o["type"], o["subtype"]) for o in wobjs], name
        for o in objs:
            h = dabgpu.mot_header_parse(d[int(o["header_offset"]):int(o["header_offset"]) + int(o["header_bytes"])])
            assert h["body_size"] == int(o["body_bytes"])
        seen += 1
    assert seen >= 20
    # what the check refuses, and a table too small: nothing is written
    L = dabgpu.lib()
    good = synth.mot_directory([(1, header(1)), (2, header(2))])
    info, out, n = np.full(8, -5, np.int32), np.full((4, 8), -5, np.int32), C.c_int(-5)
    bad = [good[:-1], good + b"\x00", synth.mot_directory([(1, header(1))], compressed=True), good[:12], synth.mot_directory([(i, header(0)) for i in range(257)])]
    for d in bad:
        assert R.parse_directory(d) in (None, "too_large")
        buf = np.frombuffer(d, np.uint8)
        assert L.dabgpu_mot_directory_parse(buf.ctypes.data, len(d), info.ctypes.data, out.ctypes.data, 4, C.byref(n)) == ARG
    buf = np.frombuffer(good, np.uint8)
    assert L.dabgpu_mot_directory_parse(buf.ctypes.data, len(good), info.ctypes.data, out.ctypes.data, 1, C.byref(n)) == CAPACITY
    assert L.dabgpu_mot_directory_parse(None, len(good), info.ctypes.data, out.ctypes.data, 4, C.byref(n)) == ARG
    assert L.dabgpu_mot_directory_parse(buf.ctypes.data, len(good), info.ctypes.data, out.ctypes.data, 4, None) == ARG
    assert (info == -5).all() and (out == -5).all() and n.value == -5
    assert L.dabgpu_mot_directory_parse(buf.ctypes.data, len(good), info.ctypes.data, out.ctypes.data, 2, C.byref(n)) == 0 and n.value == 2 and info[0] == 2


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_host_equals_the_reference(built, name):
    """each stream in one call: the reference itself reports what the stream is about and the objects that were sent; then
    slots, d_directory and counters of the host twin equal the reference's"""
    st = streams()[name]
    sp = spec_of(st)
    want = wanted(name)
    for key, value in st["counts"].items():
        assert count_of(want[2], key) == value, (name, key, count_of(want[2], key), want[2])
    assert [(int(r["transport_id"][0]), h, b) for r, h, b in want[0]] == st["objects"], name
    got = call(HostMemory(), [sp], len(sp["frames"]))[0]
    assert same(got, want), name + explain(got, want)
    assert set(STREAM_NAMES) == set(streams())


def test_two_full_assemblies_are_emitted_by_consecutive_packets_in_assembly_order(built):
    objs, _d, res = wanted("bodies first, directory out of order")
    where = [(int(r["frame"][0]), int(r["slot"][0])) for r, _h, _b in objs]
    assert len(set(where)) == 3 and where == sorted(where) and [int(r["transport_id"][0]) for r, _h, _b in objs] == [0x200, 0x201, 0x202]
    # the three attempts follow three consecutive followed packets: no followed packet lies between them
    sp = spec_of(streams()["bodies first, directory out of order"])
    followed = []
    for k, fr in enumerate(sp["frames"]):
        pos = 0
        while pos < 8:
            Ls = (int(fr[24 * pos]) >> 6) + 1
            if ((int(fr[24 * pos]) & 3) << 8 | int(fr[24 * pos + 1])) == ADDR:
                followed.append((k, pos))
            pos += Ls
    assert count_of(res, "slots_bad") == 0 and len(followed) == count_of(res, "packets_followed")
    i = followed.index(where[0])
    assert followed[i:i + 3] == where


def run_cut(st, cuts, against=None):
    """the stream in calls that end at `cuts` (and its end), state and arena handed on; each call is held to the reference's
    call on the same frames -> (objects of all calls, last directory, per-call results, last state)"""
    state, arena, at, objs, results, directory = None, None, 0, [], [], None
    n = len(st["frames"])
    for end in list(cuts) + [n]:
        sp = spec_of(st, at, end, state=state, arena=arena)
        r = call(HostMemory(), [sp], end - at)[0]
        if against is not None:
            want = ref_call(against, spec_of(st), at, end)
            assert same(r, want), (cuts, end) + (explain(r, want),)
        state, arena, at = r["state"], r["arena"], end
        objs += r["objects"]
        if int(r["result"]["directories_completed"][0]):              # (the last one of the call: its own first bytes say how long it is)
            directory = r["directory"][:int.from_bytes(r["directory"][:4], "big") & 0x3FFFFFFF]
        results.append(r["result"])
    return objs, directory, results, state


SUMMED = [k for k in R.COUNTERS if not k.startswith("directory_")]


def totals(results):
    out = {k: sum(int(r[k][0]) for r in results) for k in SUMMED}
    out.update(PR.total([r["head"] for r in results]))
    out.update({k: int(results[-1][k][0]) for k in R.COUNTERS if k.startswith("directory_")})
    return out


def strip(objs):
    """objects without where in their call they were emitted"""
    return [(int(r["transport_id"][0]), int(r["content_type"][0]), int(r["content_subtype"][0]), int(r["directory_id"][0]), h, b) for r, h, b in objs]


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_cut_into_two_and_three_calls_at_every_frame_boundary(built, name):
    """each stream cut into two calls at EVERY frame boundary and into three at every pair of neighbouring ones, state and
    arena carried: groups, directories and objects span the calls.  Every call equals the reference's call on the same
    frames; objects, last directory and summed counters equal the uncut run's, except where a call's own slots make the cut
    visible (max_objects: a deferred object is delivered by the next call), which the reference decides"""
    st = streams()[name]
    n = len(st["frames"])
    whole = run_cut(st, [])
    want = wanted(name)
    assert strip(whole[0]) == strip(want[0]) and totals(whole[2]) == totals([want[2]])
    for cuts in [[k] for k in range(0, n + 1)] + [[k, k + 1] for k in range(1, n - 1)]:
        got = run_cut(st, cuts, against=receiver(spec_of(st)))
        if st.get("cut_visible"):
            continue
        assert strip(got[0]) == strip(whole[0]) and got[1] == whole[1] and totals(got[2]) == totals(whole[2]), (name, cuts)
        assert got[3].tobytes() == whole[3].tobytes(), (name, cuts)


def test_a_deferred_object_is_delivered_by_the_next_call(built):
    st = streams()["more objects than slots"]
    n = len(st["frames"])
    rx = receiver(spec_of(st))
    objs, _d, results, _s = run_cut(st, [n - 1], against=rx)
    assert [int(r["transport_id"][0]) for r, _h, _b in objs] == [0x900, 0x901]
    assert int(results[0]["objects_deferred"][0]) == 1 and [int(r["objects_written"][0]) for r in results] == [1, 1]
    # and with one frame a call every object arrives, one call after the other
    objs, _d, results, _s = run_cut(st, list(range(1, n)), against=receiver(spec_of(st)))
    assert [int(r["transport_id"][0]) for r, _h, _b in objs] == [0x900, 0x901, 0x902]


def test_a_foreign_or_corrupted_state_record_is_a_fresh_start(built):
    name = "three cycles"
    st = streams()[name]
    rng = np.random.default_rng(7)
    want = wanted(name)
    n, nb = len(st["frames"]), dabgpu.packet_carousel_state_bytes()
    mid = call(HostMemory(), [spec_of(st, 0, 3)], 3)[0]["state"]
    assert mid.any() and not same(call(HostMemory(), [spec_of(st, state=mid)], n)[0], want)      # (ours is taken up)
    for k in range(40):
        state = rng.integers(0, 256, nb, dtype=np.uint8)
        if k % 2:                                                     # nearly ours: a record of this library's with one bit changed
            state = mid.copy()
            state[rng.integers(0, state.size)] ^= 1 << rng.integers(0, 8)
        got = call(HostMemory(), [spec_of(st, state=state)], n)[0]    # (whatever it holds: nothing outside the outputs is written)
        if k % 2 == 0:
            assert same(got, want), k
    # ours, but written for other sizes: each of the three; and ours with a size, a flag or a reserved word spoilt
    foreign = [call(HostMemory(), [spec_of(st, 0, 3, **{key: DEFAULTS[key] + 16})], 3)[0]["state"] for key in ("directory_capacity", "assemblies", "object_capacity")]
    for at, value in ((176, 0xFF), (180, 9), (184, 1), (199, 1), (216, 1), (0, 1)):
        state = mid.copy()
        state[at] ^= value
        foreign.append(state)
    for k, state in enumerate(foreign + [np.zeros(nb, np.uint8)]):
        assert same(call(HostMemory(), [spec_of(st, state=state)], n)[0], want), k


def refusal_specs():
    st = streams()["plain, directory in 3"]
    return [spec_of(st), spec_of(st, stride=3 * st["bitrate"] + 8)], len(st["frames"])


def _set(i, **kw):
    def m(entries):
        for k, v in kw.items():
            setattr(entries[i], k, v(getattr(entries[i], k)) if callable(v) else v)
    return m


BAD_ENTRIES = [
    _set(0, bitrate_kbps=4), _set(1, bitrate_kbps=68), _set(0, bitrate_kbps=520), _set(1, in_stride=lambda v: 3 * 64 - 1), _set(0, address=0), _set(1, address=1024),
    _set(0, d_in=None), _set(1, d_state_out=None), _set(0, d_arena=None), _set(1, d_result=None), _set(0, d_state_out=lambda v: v + 8),
    _set(1, d_arena=lambda v: v + 4), _set(0, d_objects=lambda v: v + 8), _set(1, d_result=lambda v: v + 2), _set(0, d_objects=None),
    _set(1, object_stride=16), _set(0, object_stride=1032), _set(1, max_objects=-1), _set(0, max_objects=1 << 21, object_stride=1024),
    # the new fields outside their ranges, the arena below its size, no directory buffer
    _set(0, directory_capacity=15), _set(1, directory_capacity=(1 << 20) + 1), _set(0, assemblies=0), _set(1, assemblies=33),
    _set(0, object_capacity=-1), _set(1, object_capacity=256 * 8191 + 1), _set(0, arena_bytes=lambda v: v - 1), _set(1, assemblies=5),
    _set(0, directory_capacity=1025), _set(1, object_capacity=513), _set(0, d_directory=None), _set(1, d_directory=lambda v: v + 8),
]


def test_refused_calls_leave_every_output_alone(built):
    specs, n = refusal_specs()
    for m in BAD_ENTRIES:
        call(HostMemory(), specs, n, mutate=m, refused=ARG)
    L = dabgpu.lib()
    assert L.dabgpu_packet_carousel_host(None, 1, 1) == ARG and L.dabgpu_packet_carousel_host(None, -1, 1) == ARG
    assert L.dabgpu_packet_carousel_host(None, 0, 1) == 0 and L.dabgpu_packet_carousel_dev(None, None, 0, 0, None) == ARG
    # the two state records may not overlap by the size of THIS call's record
    nb = dabgpu.packet_carousel_state_bytes()
    st = streams()["plain, directory in 3"]
    call(HostMemory(), [spec_of(st, state=np.zeros(nb, np.uint8))], n, refused=ARG,
         mutate=lambda entries: setattr(entries[0], "d_state_in", entries[0].d_state_out + nb - 16))
    got = call(HostMemory(), specs, n)
    assert all(same(r, wanted("plain, directory in 3")) for r in got)


# ---- device code
def test_the_new_instantiation_neither_spills_nor_uses_scratch(built, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the device assembly cannot be checked")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "packet_carousel_kernels.hip" in mk
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    out = tmp_path / "packet_carousel_kernels.s"
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "packet_carousel_kernels.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    md = kernel_metadata(out.read_text())
    assert len(md) == 1 and all("packet_walk_kernel" in k and "CarouselWalk" in k for k in md)
    for k, v in md.items():
        print("%s: vgprs %s, sgprs %s, LDS %s bytes" % (k, v.get("vgpr_count"), v.get("sgpr_count"), v.get("group_segment_fixed_size")))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["group_segment_fixed_size"] <= 8192


def test_control_under_sanitizers_on_random_and_mutated_frames(built, tmp_path):
    """tests/packet_carousel_fuzz.cpp: the control walk on random and mutated frames and state records, the arena, d_directory
    and the slots exactly sized, every copy order's bounds asserted before it is executed; a stand-alone program built with
    the host compiler under AddressSanitizer and UBSan and run as a child process"""
    exe = str(tmp_path / "packet_carousel_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "packet_carousel_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "30000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "frames=30000" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = dict(kv.split("=") for kv in r.stdout.split())
    print(r.stdout)
    for key in ("written", "directories", "mismatched", "evicted", "stale", "unlisted", "repeated", "dropped", "deferred", "fresh"):
        assert int(got[key]) > 0, (key, r.stdout)


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


def all_specs(n_cifs=None):
    """every stream as one entry of one table: in_stride beyond the frame and frames off their 16-byte and 4-byte boundaries by
    turns, the three entries of the shared sub-channel naming the same frames"""
    specs, shared, index = [], {}, {}
    for e, name in enumerate(STREAM_NAMES):
        st = streams()[name]
        sp = spec_of(st, 0, n_cifs)
        index[name] = e
        if st.get("share") and st["share"] != name:
            shared[e] = index[st["share"]]
            sp.update(stride=specs[shared[e]]["stride"])              # (the same frames: the same in_stride)
        else:
            sp.update(stride=3 * st["bitrate"] + [0, 2, 16, 5][e % 4], in_off=[0, 8, 4, 1, 13][e % 5])
        specs.append(sp)
    return specs, shared


def padded(specs, n):
    """the specs with frames of 0xFF behind what they have, up to n rows (a call reads n_cifs rows of every entry)"""
    out = []
    for sp in specs:
        fr = sp["frames"]
        if len(fr) < n:
            fr = np.concatenate([fr, np.full((n - len(fr), fr.shape[1]), 0xFF, np.uint8)])
        out.append(dict(sp, frames=fr))
    return out


@pytest.mark.gpu
def test_gpu_every_stream_in_one_call(pctx):
    """all streams in ONE call of 68 logical frames (rows of 0xFF behind the shorter streams): bit rates 8, 64, 72 and 512,
    three entries on one d_in, in_stride beyond 3 R, d_in off 16 and off 4 bytes: slots, d_directory, counters, state record
    and arena equal the reference and the host call"""
    specs, shared = all_specs()
    specs = padded(specs, 68)
    wants = [ref_call(receiver(sp), sp) for sp in specs]
    got = call(DeviceMemory(pctx), specs, 68, shared=shared)
    host = call(HostMemory(), specs, 68, shared=shared)
    for name, g, h, w in zip(STREAM_NAMES, got, host, wants):
        assert same(g, w), name + explain(g, w)
        assert same(h, w), name
        assert g["state"].tobytes() == h["state"].tobytes() and (g["arena"] == h["arena"]).all(), name
    assert sum(len(g["objects"]) for g in got) >= 60


@pytest.mark.gpu
@pytest.mark.parametrize("n_cifs", [0, 1, 7])
def test_gpu_short_calls(pctx, n_cifs):
    """calls of 0, 1 and 7 logical frames (68 is the call above), every entry"""
    specs, shared = all_specs()
    specs = [dict(sp, frames=sp["frames"][:n_cifs]) for sp in padded(specs, n_cifs)]
    wants = [ref_call(receiver(sp), sp) for sp in specs]
    got = call(DeviceMemory(pctx), specs, n_cifs, shared=shared)
    host = call(HostMemory(), specs, n_cifs, shared=shared)
    for name, g, h, w in zip(STREAM_NAMES, got, host, wants):
        assert same(g, w), name + explain(g, w)
        assert g["state"].tobytes() == h["state"].tobytes() and (g["arena"] == h["arena"]).all(), name


@pytest.mark.gpu
def test_gpu_130_entries_in_one_table(pctx):
    """130 entries: thirteen streams of at most 12 frames, ten times over with K and the capacities varied, each with outputs
    of its own"""
    names = [n for n in STREAM_NAMES if len(streams()[n]["frames"]) <= 12 and "exactly" not in n and "one byte more" not in n and "K " not in n and
             not n.startswith("shared")][:13]
    assert len(names) == 13, names
    specs = padded([spec_of(streams()[n], stride=3 * streams()[n]["bitrate"] + 3 * (k % 2), assemblies=[4, 1, 32, 7, 2][k % 5] if k else streams()[n].get("assemblies", 4),
                            object_capacity=streams()[n].get("object_capacity", 512) + 16 * (k % 3),
                            directory_capacity=streams()[n].get("directory_capacity", 1024) + 7 * (k % 4)) for k in range(10) for n in names], 12)
    got = call(DeviceMemory(pctx), specs, 12)
    for k, (g, sp) in enumerate(zip(got, specs)):
        w = ref_call(receiver(sp), sp)
        assert same(g, w), (k, names[k % 13]) + (explain(g, w),)


@pytest.mark.gpu
def test_gpu_two_calls_back_to_back_with_the_state_on_the_device(pctx):
    """streams in two calls enqueued one behind the other, nothing waiting in between: the state record of the first is the
    second's input, the arena stays in place.  The cut lies inside a directory and inside an object ("N 256",
    "a body of more than 64 KiB", ...), and "more objects than slots" is cut where the second call delivers the deferred
    object.  Each call equals the reference's"""
    import torch
    nb = dabgpu.packet_carousel_state_bytes()
    cuts = {"N 256": 8, "a body of more than 64 KiB": 20, "directory change": 3, "three cycles": 4, "segment sizes": 6,
            "more objects than slots": len(streams()["more objects than slots"]["frames"]) - 1}
    bufs, entries = {}, [[], []]
    for name, cut in cuts.items():
        sp = spec_of(streams()[name])
        n = len(sp["frames"])
        assert 0 < cut < n
        b = bufs[name] = dict(sp=sp, cut=cut, frames=torch.from_numpy(sp["frames"]).cuda(), states=torch.zeros((2, nb), dtype=torch.uint8, device="cuda"),
                              arena=torch.full((dabgpu.packet_carousel_arena_bytes(*sizes_of(sp)),), FILL, dtype=torch.uint8, device="cuda"),
                              objects=torch.full((2, sp["max_objects"], sp["object_stride"]), FILL, dtype=torch.uint8, device="cuda"),
                              directory=torch.full((2, (sp["directory_capacity"] + 15) // 16 * 16), FILL, dtype=torch.uint8, device="cuda"),
                              results=torch.zeros((2, NB), dtype=torch.uint8, device="cuda"))
        for i, (a, e) in enumerate(((0, cut), (cut, n))):
            entries[i].append(dabgpu.PacketCarouselEntry(
                b["frames"].data_ptr() + a * 3 * sp["bitrate"], 3 * sp["bitrate"], sp["bitrate"], ADDR, 0, sp["assemblies"],
                None if i == 0 else b["states"][0].data_ptr(), b["states"][i].data_ptr(), b["arena"].data_ptr(), b["arena"].numel(),
                b["objects"][i].data_ptr(), sp["object_stride"], sp["max_objects"], sp["object_capacity"], b["directory"][i].data_ptr(),
                sp["directory_capacity"], 0, b["results"][i].data_ptr()))
    # one table per call needs one n_cifs: the streams are cut at different frames, so each stream is its own pair of calls,
    # all enqueued before anything is waited for
    for j, name in enumerate(cuts):
        b = bufs[name]
        pctx.packet_carousel_dev([entries[0][j]], b["cut"])
        pctx.packet_carousel_dev([entries[1][j]], len(b["sp"]["frames"]) - b["cut"])
    pctx.sync()
    for name, b in bufs.items():
        sp, rx = b["sp"], receiver(b["sp"])
        for i, (a, e) in enumerate(((0, b["cut"]), (b["cut"], len(sp["frames"])))):
            wo, wd, wr = ref_call(rx, sp, a, e)
            res = b["results"][i].cpu().numpy().view(dabgpu.PACKET_CAROUSEL_RESULT_DTYPE)
            assert res.tobytes() == wr.tobytes(), (name, i, res, wr)
            raw = b["objects"][i].cpu().numpy()
            for k, (rec, h, body) in enumerate(wo):
                assert raw[k, :32].tobytes() == rec.tobytes() and raw[k, 32:32 + len(h)].tobytes() == h, (name, i, k)
                assert raw[k, 32 + len(h):32 + len(h) + len(body)].tobytes() == body and (raw[k, 32 + len(h) + len(body):] == FILL).all(), (name, i, k)
            assert (raw[len(wo):] == FILL).all()
            d = b["directory"][i].cpu().numpy()
            n_d = len(wd) if wd is not None else 0
            assert d[:n_d].tobytes() == (wd or b"") and (d[n_d:] == FILL).all(), (name, i)
    # an object and a directory span the cut; the deferred object arrives in the second call
    res = bufs["more objects than slots"]["results"].cpu().numpy().view(dabgpu.PACKET_CAROUSEL_RESULT_DTYPE)
    assert int(res[0]["objects_deferred"][0]) == 1 and [int(r["objects_written"][0]) for r in res] == [1, 1]
    res = bufs["N 256"]["results"].cpu().numpy().view(dabgpu.PACKET_CAROUSEL_RESULT_DTYPE)
    assert int(res[0]["directories_completed"][0]) == 0 and int(res[1]["directories_completed"][0]) == 1 and int(res[0]["head"]["mot"]["segments_placed"][0]) > 0
    res = bufs["a body of more than 64 KiB"]["results"].cpu().numpy().view(dabgpu.PACKET_CAROUSEL_RESULT_DTYPE)
    assert int(res[0]["objects_written"][0]) == 0 and int(res[1]["objects_written"][0]) == 1 and int(res[0]["head"]["mot"]["segments_placed"][0]) > 10


@pytest.mark.gpu
def test_gpu_refused_calls_leave_every_output_alone(pctx):
    specs, n = refusal_specs()
    for m in BAD_ENTRIES:
        call(DeviceMemory(pctx), specs, n, mutate=m, refused=ARG)
    pctx.packet_carousel_dev([], 4)                                   # nothing to do is not an error
    got = call(DeviceMemory(pctx), specs, n)
    assert all(same(r, wanted("plain, directory in 3")) for r in got)


# ---- end to end
E2E_SEED = 3
E2E_DABPLUS = [("Radio One", 0xC221, 3, 0, 3, 64, 0)]
E2E_OBJECTS = [(0x501, header(150, b"logo32.png"), image(150, 77)), (0x502, header(90, b"logo128.png"), image(90, 78))]
E2E_SCID, E2E_SUBCH, E2E_START = 0x123, 9, 48


def e2e_ensemble():
    """one ensemble: a DAB+ service of 64 kbit/s, and a packet-mode sub-channel of 32 kbit/s that carries the carousel (a
    directory and two small objects) twice in its cycle of 20 logical frames"""
    d, b = synth.mot_carousel_groups(0x60, E2E_OBJECTS, 60)
    cycle = d + flat(b)
    pk = synth.packetise(cycle + cycle, ADDR, sizes=(4,))
    while len(pk) % 4:                                                # (command packets, so that the continuity index goes on where the cycle wraps)
        pk.append(synth.packet(ADDR, b"\x00", 1, ci=len(pk), command=True))
    frames = synth.packet_frames(32, [pk], n_frames=20)
    assert frames.shape == (20, 96), frames.shape
    service = ("Logos", 0xD301, E2E_SUBCH, 0, 3, 32, E2E_START, [(E2E_SCID, ADDR, synth.DSCTY_MOT, 0)], frames, 0)
    return synth.ServiceEnsemble(E2E_SEED, E2E_DABPLUS, n_frames=5, extras=False, packet_services=[service]), frames, len(cycle)


def test_end_to_end_multiplex_carries_the_carousel(built):
    """what the GPU test will receive: the reference receiver on the transmitted logical frames, two cycles of them"""
    ens, frames, n_groups = e2e_ensemble()
    comps = dabgpu.fig_packet_components(ens.fibs, np.ones((5, 12), np.uint8))
    assert [(c.subchid, c.packet_address, c.dscty, c.dg_flag) for c in comps] == [(E2E_SUBCH, ADDR, 60, 0)]
    objs, d, res = R.Receiver(256, 2, 256, ADDR).call(np.concatenate([frames, frames]), 32, 4, 512)
    assert [(int(r["transport_id"][0]), h, b) for r, h, b in objs] == E2E_OBJECTS and count_of(res, "slots_bad") == 0
    assert count_of(res, "groups_repeated") == 3 * n_groups and count_of(res, "continuity_breaks") == 0 and count_of(res, "directories_completed") == 1


@pytest.mark.gpu
def test_gpu_end_to_end_iq_to_objects(pctx):
    """IQ of 16 transmission frames of that ensemble -> front end -> FIC pass -> fig_subchannels and fig_packet_components ->
    decode_ensembles_dev -> packet_carousel_dev behind it on the same stream, nothing waiting in between: both objects as
    sent, each exactly once, and not one packet lost (so the test cannot pass by losing the second copy)"""
    import torch
    dev = torch.device("cuda", 0)
    fps, L, FB = 16, 76 * 2552, dabgpu.NB_FRAME_BITS
    ens, frames, n_groups = e2e_ensemble()
    tx = ens.iq()
    c = pctx
    c.streams_reset(1)
    rx = synth.channel(tx[np.arange(fps) % 5].ravel(), snr_db=20.0, rng=np.random.default_rng(12)).reshape(fps, -1)
    d_iq = torch.from_numpy(np.ascontiguousarray(rx[:, synth.NB_NULL:synth.NB_NULL + L]).astype(np.complex64)).to(dev)
    d_soft = torch.zeros((fps, FB), dtype=torch.int8, device=dev)
    c.ofdm_demod_streams_dev(d_iq.data_ptr(), L, 1, fps, 0.9, d_soft.data_ptr(), None, None)
    fib = torch.zeros((fps, 12, 32), dtype=torch.uint8, device=dev)
    ok = torch.zeros((fps, 12), dtype=torch.uint8, device=dev)
    c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), [[]], None, None, None, None)
    c.sync()
    fib_h, ok_h = fib.cpu().numpy(), ok.cpu().numpy()
    assert ok_h.all()
    plan = dabgpu.fig_subchannels(fib_h, ok_h)
    comps = [a for a in dabgpu.fig_packet_components(fib_h, ok_h) if a.dscty == dabgpu.DSCTY_MOT and a.dg_flag == 0]
    assert [sc.bitrate_kbps for sc in plan] == [64, 32] and len(comps) == 1 and comps[0].packet_address == ADDR
    j = [sc.start_address for sc in plan].index(comps[0].start_address)
    br, n_cifs = plan[j].bitrate_kbps, 4 * fps
    hist = [torch.zeros((15, sc.length * 64), dtype=torch.int8, device=dev) for sc in plan]
    outs = [torch.zeros((n_cifs, sc.bitrate_kbps * 3), dtype=torch.uint8, device=dev) for sc in plan]
    sizes = (256, 2, 256)
    state = torch.zeros(dabgpu.packet_carousel_state_bytes(), dtype=torch.uint8, device=dev)
    arena = torch.zeros(dabgpu.packet_carousel_arena_bytes(*sizes), dtype=torch.uint8, device=dev)
    slots = torch.full((4, 512), FILL, dtype=torch.uint8, device=dev)
    directory = torch.full((256,), FILL, dtype=torch.uint8, device=dev)
    result = torch.zeros(NB, dtype=torch.uint8, device=dev)
    c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), [plan], None, [[h.data_ptr() for h in hist]],
                           [[o.data_ptr() for o in outs]], None)
    # (the time de-interleaver starts empty: the first 15 logical frames of a sub-channel are not decodable, whatever follows
    # them; the call is given the frames from the 16th on, and on those not one packet may be lost)
    skip = 16
    c.packet_carousel_dev([dabgpu.PacketCarouselEntry(outs[j].data_ptr() + skip * 3 * br, 3 * br, br, comps[0].packet_address, comps[0].fec_scheme,
                                                      sizes[1], None, state.data_ptr(), arena.data_ptr(), arena.numel(), slots.data_ptr(), 512, 4,
                                                      sizes[2], directory.data_ptr(), sizes[0], 0, result.data_ptr())], n_cifs - skip)
    c.sync()                                                          # (the only wait behind the decode call)
    res = result.cpu().numpy().view(dabgpu.PACKET_CAROUSEL_RESULT_DTYPE)
    raw = slots.cpu().numpy()
    # the reference on the frames the decoder wrote: not one slot is bad there, so no copy was lost on the way
    wo, wd, wr = R.Receiver(*sizes, ADDR, comps[0].fec_scheme).call(outs[j].cpu().numpy()[skip:], br, 4, 512)
    assert count_of(wr, "slots_bad") == 0 and count_of(wr, "continuity_breaks") == 0 and count_of(wr, "groups_crc_failed") == 0, wr
    assert res.tobytes() == wr.tobytes(), (res, wr)
    assert count_of(res, "objects_written") == 2 and count_of(res, "groups_repeated") >= n_groups and count_of(res, "cifs") == n_cifs - skip, res
    for k, (tid, h, body) in enumerate(E2E_OBJECTS):
        rec = raw[k, :32].copy().view(dabgpu.MOT_CAROUSEL_OBJECT_DTYPE)
        assert rec.tobytes() == wo[k][0].tobytes() and int(rec["transport_id"][0]) == tid and int(rec["directory_id"][0]) == 0x60
        assert raw[k, 32:32 + len(h)].tobytes() == h and raw[k, 32 + len(h):32 + len(h) + len(body)].tobytes() == body
        assert (raw[k, 32 + len(h) + len(body):] == FILL).all() and dabgpu.mot_header_parse(h)["body_size"] == len(body)
    assert (raw[2:] == FILL).all()
    d = directory.cpu().numpy()
    assert d[:len(wd)].tobytes() == wd and (d[len(wd):] == FILL).all()
    info, listed = dabgpu.mot_directory_parse(wd)
    assert int(info["objects"]) == 2 and [int(o["transport_id"]) for o in listed] == [0x501, 0x502]
