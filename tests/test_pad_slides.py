"""dabgpu_mot_slides_dev / dabgpu_mot_slides_host (the slideshow objects of every followed DAB+ service, from the X-PAD of
its access units) and dabgpu_mot_header_parse, against tests/mot_reference.py: slides, counters byte for byte and count
for count -- no tolerance anywhere -- every output between sentinel bytes.

The cases are streams of at most 16 super-frames (STREAMS), each a sequence of scenarios that begin on a super-frame: the
CPU tests feed them scenario by scenario through dabgpu_mot_slides_host, state and arena handed on, and check what each
scenario is about; the GPU test takes all of them in one ragged call.  The transmit side is dabgpu/synth.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import mot_reference as M
import pad_reference as P
from conftest import ROOT
from test_device_asm import CSRC, kernel_metadata
from test_pad_labels import NO_PAD, RANDOM, clear_crc_bit, firecode_fails, starts_out_of_range, superframes

ARG, CAPACITY = -1, -6
FILL, GAP = 0xA7, 64


# ------------------------------------------------------------------------------------------------ building streams
def image(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def obj(tid, body, name, seg, hseg=None, extra=(), **kw):
    """-> (header bytes, body bytes, data groups: header's, then body's)"""
    header = synth.slide_header(len(body), name, extra=extra)
    return header, bytes(body), synth.mot_object_groups(tid, header, body, seg, hseg, **kw)


class Scenario:
    def __init__(self, name, pads, slides=(), counts=None, damage=None, max_slides=4, slide_stride=None, rows=None):
        """slides: (transport id, header, body) of the objects the scenario completes, in order; counts: counters of the
        scenario that the reference must report (a subset); damage(status rows of the scenario): reception losses;
        rows(s) -> (data, status): super-frames laid out by hand (unit_rows) in the place of `pads`"""
        self.name, self.pads, self.slides, self.counts, self.damage = name, pads, list(slides), counts or {}, damage
        self.max_slides, self.slide_stride, self.rows = max_slides, slide_stride, rows


def sent(*objs):
    return [(tid, o[0], o[1]) for tid, o in objs]


def sized_object(tid, hbytes, bbytes, seed, seg=2048, hseg=2048):
    """an object whose header has exactly hbytes >= 16 (an unknown parameter fills it up): in its slot the body begins
    32 + hbytes bytes in"""
    name = synth.mot_param(synth.MOT_CONTENT_NAME, b"\xf0cap")
    header = synth.mot_header(bbytes, 2, 1, [name, synth.mot_param(0x3A, bytes(hbytes - 7 - len(name) - 3), pli=3, long_length=True)])
    assert len(header) == hbytes
    body = image(bbytes, seed)
    return header, body, synth.mot_object_groups(tid, header, body, seg, hseg)


def placed_object(tid, size, last, eu0, eu1, seed):
    """an object whose body is one segment of `size` bytes and a last one of `last`, in data groups whose end-user address has
    eu0 and eu1 bytes: the segments lie 9 + eu bytes into the group buffer and go to body offsets 0 and `size`"""
    body = image(size + last, seed)
    header = synth.slide_header(len(body), b"placed %x" % tid)
    groups = [synth.mot_group(3, tid, 0, True, header), synth.mot_group(4, tid, 0, False, body[:size], end_user=bytes(eu0)),
              synth.mot_group(4, tid, 1, True, body[size:], end_user=bytes(eu1), continuity=1)]
    return header, body, groups


NO_AUDIO = b"\x21\x00\x00"                                            # an access unit with a channel pair element in front


def unit(fields, n=None, behind=b""):
    """an access unit laid out by hand: the data stream element whose PAD of n bytes (default: no more than needed) carries
    these sub-fields [(type, data)], and what follows the element"""
    return synth.dse(synth.fields_pads([fields], n=n)[0]) + bytes(behind)


def unit_rows(units, claim=None, first=11):
    """Scenario(rows=): super-frames whose access units are given byte for byte, at most seven each (bytes without the CRC,
    or (bytes, what lies behind them where the CRC would be: at most 2 bytes)); they lie back to back from byte `first`;
    claim: what num_aus says (default: the truth).  What a data part holds besides is 0xEE."""
    def rows(s):
        data, status = np.full((len(units), 110 * s), 0xEE, np.uint8), np.zeros(len(units), P.STATUS_DTYPE)
        for k, us in enumerate(units):
            at, starts = first, [first]
            for u in us:
                au, behind = u if isinstance(u, tuple) else (u, b"")
                assert len(au) >= 1 and len(behind) <= 2
                data[k, at:at + len(au) + len(behind)] = np.frombuffer(bytes(au) + bytes(behind), np.uint8)
                at += len(au) + 2
                starts.append(at)
            assert at <= 110 * s and len(us) <= 7
            status[k]["firecode_ok"], status[k]["num_aus"], status[k]["au_crc_mask"] = 1, claim or len(us), (1 << len(us)) - 1
            status[k]["au_start"][:len(starts)] = starts
        return data, status
    return rows


def _streams():
    S = {}
    mp = synth.mot_pads
    # A: s = 8, three access units: the body's sizes
    o0, o1, o2 = obj(0x100, b"", b"empty.jpg", 32), obj(0x101, b"\x5a", b"one.jpg", 32), obj(0x102, image(32, 1), b"segment.jpg", 32)
    o3, o4 = obj(0x103, image(75, 2), b"three.jpg", 32), obj(0x104, image(40, 3), b"split header.png", 32, hseg=16)
    S["bodies"] = dict(s=8, num_aus=3, seed=31, body_capacity=4096, scenarios=[
        Scenario("body of 0 bytes", mp(o0[2], 5), sent((0x100, o0)), dict(groups_ok=2, segments_placed=2, objects_completed=1, slides_written=1)),
        Scenario("body of 1 byte", mp(o1[2], 5), sent((0x101, o1)), dict(groups_ok=2, lengths_ok=2)),
        Scenario("body of exactly one segment", mp(o2[2], 5), sent((0x102, o2)), dict(groups_ok=2)),
        Scenario("three segments, the last one shorter", mp(o3[2], 5), sent((0x103, o3)), dict(groups_ok=4, segments_placed=4)),
        Scenario("header in two segments", mp(o4[2], 5), sent((0x104, o4)), dict(groups_ok=len(o4[2]), groups_malformed=0)),
    ])
    assert len(o3[2]) == 4 and len(o4[2]) >= 4
    # B: s = 24, six access units: a small object at each variable length index
    idx = [obj(0x200 + i, image(20 + i, 10 + i), b"index %d" % i, 20 + i) for i in range(8)]
    esc = obj(0x304, image(30, 24), b"escape", 64)
    S["indices"] = dict(s=24, num_aus=6, seed=32, body_capacity=256, scenarios=[
        Scenario("length index %d" % i, mp(idx[i][2], i), sent((0x200 + i, idx[i])), dict(groups_ok=2, slides_written=1)) for i in range(8)] + [
        Scenario("PAD of 300 bytes: the escape byte", mp(esc[2], 4, n=300), sent((0x304, esc)), dict(groups_ok=2, pad_malformed=0))])
    # C: s = 8, four access units: X-PAD layouts
    big, both = obj(0x300, image(200, 20), b"spans.jpg", 200), obj(0x301, image(60, 21), b"beside a label", 64)
    less, behind = obj(0x302, image(70, 22), b"ci-less", 80), obj(0x303, image(50, 23), b"behind", 64)
    S["layouts"] = dict(s=8, num_aus=4, seed=33, body_capacity=4096, scenarios=[
        Scenario("a group that spans super-frames", mp(big[2], 3), sent((0x300, big)), dict(groups_ok=2)),
        Scenario("a slide and a label in one PAD", mp(both[2], 4, after=synth.dls_fields(LABEL_GROUPS[0], 4)), sent((0x301, both)), dict(groups_ok=2)),
        Scenario("CI-less continuation of type 13", mp(less[2], 4, ci_less=True), sent((0x302, less)), dict(groups_ok=2, fields_ignored=0)),
        Scenario("a 12 behind a 2 / 3 in one list", mp(behind[2], 4, before=synth.dls_fields(LABEL_GROUPS[1], 2)), sent((0x303, behind)), dict(groups_ok=2)),
    ])
    # D: s = 8, three access units: the length indicator
    d0, d1 = obj(0x400, image(20, 30), b"length", 64), obj(0x401, image(20, 31), b"no length", 64)
    bad = synth.mot_fields(d0[2][:1], 5)
    bad[0][0] = (synth.XPAD_DGLI, synth.dgli(len(d0[2][0]), good=False))
    short_li = [synth.pad_field(synth.xpad_short(synth.dgli(40)[:3], synth.XPAD_DGLI), 1, 1)]
    S["lengths"] = dict(s=8, num_aus=3, seed=34, body_capacity=4096, scenarios=[
        Scenario("an indicator with a bad CRC, then the object", synth.fields_pads(bad) + mp(d0[2], 5), sent((0x400, d0)),
                 dict(lengths_ignored=1, groups_no_length=1, lengths_ok=2, groups_ok=2)),
        Scenario("type 12 with no length", mp(d1[2], 5, with_length=False), [], dict(groups_no_length=2, groups_ok=0, xpad_bytes=0)),
        Scenario("a sub-field too short for the indicator", short_li + mp(d1[2], 5), sent((0x401, d1)), dict(lengths_ignored=1, lengths_ok=2)),
    ])
    # E: s = 24, six access units: the largest segment
    huge = obj(0x500, image(8191, 40), b"largest segment.jpg", 8191)
    assert len(huge[2]) == 2 and len(huge[2][1]) == 8191 + 11
    S["maxlen"] = dict(s=24, num_aus=6, seed=35, body_capacity=8191, scenarios=[
        Scenario("a segment of 8191 bytes", mp(huge[2], 7, per_au=4), sent((0x500, huge)), dict(groups_ok=2, xpad_bytes=sum(map(len, huge[2]))),
                 slide_stride=8192 + 128)])
    # F: s = 8, three access units: data groups
    f0, f1, f2 = obj(0x600, image(30, 50), b"crc", 64), obj(0x601, image(30, 51), b"types", 64), obj(0x602, image(30, 52), b"no id", 64)
    f3 = obj(0x603, image(30, 53), b"extended", 64, extension=0xBEEF, end_user=b"\x01\x02\x03")
    broken = bytearray(f0[2][1])
    broken[12] ^= 0x10
    no_crc = synth.mot_group(4, 0x600, 0, True, f0[1], crc=False)
    others = [synth.msc_data_group(6, bytes(20), 0x601, (0, True)), synth.msc_data_group(5, bytes(20), 0x601, (0, True))]
    anon = [synth.mot_group(4, None, 0, True, f2[1]), synth.mot_group(4, None, 0, True, f2[1], user_access=True),
            synth.msc_data_group(4, bytes(20), 0x602)]
    S["groups"] = dict(s=8, num_aus=3, seed=36, body_capacity=4096, scenarios=[
        Scenario("a CRC failure, a group without CRC, then the repetition", mp([f0[2][0], bytes(broken), no_crc, f0[2][1]], 5), sent((0x600, f0)),
                 dict(groups_crc_failed=2, groups_ok=2)),
        Scenario("data group types 6 and 5", mp(others + f1[2], 5), sent((0x601, f1)), dict(groups_ignored_type=2, groups_ok=2)),
        Scenario("no transport id; no segment field", mp(anon + f2[2], 5), sent((0x602, f2)), dict(groups_no_transport_id=2, groups_malformed=1, groups_ok=2)),
        Scenario("an extension field and an end-user address", mp(f3[2], 5), sent((0x603, f3)), dict(groups_ok=2)),
    ])
    # G: s = 8, six access units: the assembly
    g0, g1, g2 = obj(0x700, image(70, 60), b"order", 32), obj(0x701, image(70, 61), b"last first", 32), obj(0x702, image(70, 62), b"sizes", 32)
    g3, g4, g5 = obj(0x703, image(70, 63), b"abandoned", 32), obj(0x704, image(40, 64), b"instead", 32), obj(0x705, image(40, 65), b"twice", 32)
    h, b0, b1, b2 = range(4)
    odd = synth.mot_group(4, 0x702, 1, False, image(31, 66))
    S["assembly"] = dict(s=8, num_aus=6, seed=37, body_capacity=4096, scenarios=[
        Scenario("segments out of order", mp([g0[2][b1], g0[2][b0], g0[2][h], g0[2][b2]], 5), sent((0x700, g0)), dict(groups_ok=4, segments_early_last=0)),
        Scenario("the last segment first: dropped, then repeated", mp([g1[2][b2], g1[2][h], g1[2][b0], g1[2][b1], g1[2][b0], g1[2][b2]], 5), sent((0x701, g1)),
                 dict(segments_early_last=1, segments_repeated=1, groups_ok=6)),
        Scenario("a segment of another size", mp([g2[2][h], g2[2][b0], odd, g2[2][b1], g2[2][b2]], 5), sent((0x702, g2)), dict(groups_malformed=1, groups_ok=5)),
        Scenario("a new transport id in mid-object", mp(g3[2][:2] + g4[2], 5), sent((0x704, g4)), dict(groups_ok=2 + len(g4[2]), slides_written=1)),
        Scenario("the whole object twice", mp(g5[2] + g5[2], 5), sent((0x705, g5)), dict(groups_repeated=len(g5[2]), slides_written=1)),
    ])
    # H: s = 8, three access units: reception losses
    l0, l1, l2 = obj(0x800, image(50, 70), b"loss", 64), obj(0x801, image(20, 71), b"fire", 64), obj(0x802, image(20, 72), b"starts", 64)
    S["loss"] = dict(s=8, num_aus=3, seed=38, body_capacity=4096, scenarios=[
        Scenario("a lost access unit in mid-group, then the repetition", mp(l0[2] + l0[2][1:], 5), sent((0x800, l0)), damage=clear_crc_bit(1, 0),
                 counts=dict(aus_lost=1, groups_ok=2, groups_crc_failed=0)),
        Scenario("a super-frame whose Fire code fails", mp(l1[2], 5)[:3] + mp(l1[2], 5), sent((0x801, l1)), damage=firecode_fails(0), counts=dict(aus_lost=1, groups_ok=2)),
        Scenario("start addresses out of range", [None] * 6 + mp(l2[2], 5), sent((0x802, l2)), damage=starts_out_of_range, counts=dict(aus_lost=4)),
    ])
    assert len(mp(l0[2], 5)) == 5 and len(mp(l1[2], 5)) == 4
    # I: s = 24, six access units, a body capacity of 256: every cap at the cap and one beyond
    def sized(tid, hbytes, bbytes, seed):
        """an object whose header has exactly hbytes (an unknown parameter fills it up)"""
        name = synth.mot_param(synth.MOT_CONTENT_NAME, b"\xf0cap")
        fill = hbytes - 7 - len(name) - 3
        header = synth.mot_header(bbytes, 2, 1, [name, synth.mot_param(0x3A, bytes(fill), pli=3, long_length=True)])
        assert len(header) == hbytes
        body = image(bbytes, seed)
        return header, body, synth.mot_object_groups(tid, header, body, 256, 2048)
    c0, c1, c2, c3 = sized(0x900, 1024, 16, 80), sized(0x901, 1025, 16, 81), sized(0x902, 64, 256, 82), sized(0x903, 64, 257, 83)
    seg = lambda typ, tid, n: synth.mot_group(typ, tid, n, False, b"\x33")
    S["caps"] = dict(s=24, num_aus=6, seed=39, body_capacity=256, scenarios=[
        Scenario("a header of 1024 bytes", mp(c0[2], 7, per_au=4), sent((0x900, c0)), dict(objects_too_large=0), slide_stride=2048),
        Scenario("a header of 1025 bytes", mp(c1[2], 7, per_au=4), [], dict(objects_too_large=1, groups_ok=2, segments_placed=0), slide_stride=2048),
        Scenario("a body of 256 bytes", mp(c2[2], 7, per_au=4), sent((0x902, c2)), dict(objects_too_large=0)),
        Scenario("a body of 257 bytes", mp(c3[2], 7, per_au=4), [], dict(objects_too_large=1, segments_placed=2)),
        Scenario("segments 255 and 31, then 256 and 32", mp([seg(4, 0x904, 255), seg(3, 0x904, 31), seg(4, 0x905, 256), seg(4, 0x905, 0), seg(3, 0x906, 32)], 2), [],
                 dict(segments_placed=2, objects_too_large=2, groups_ok=5)),
    ])
    # J: s = 8, six access units: more completions than slots, a slot too small
    small = [obj(0xA00 + i, image(24, 90 + i), b"s%d" % i, 32) for i in range(4)]
    S["slots"] = dict(s=8, num_aus=6, seed=40, body_capacity=256, scenarios=[
        Scenario("three objects, two slots", mp(small[0][2] + small[1][2] + small[2][2], 5), sent((0xA00, small[0]), (0xA01, small[1])),
                 dict(objects_completed=3, slides_written=2, slides_dropped=1), max_slides=2),
        Scenario("a slot too small", mp(small[3][2], 5), [], dict(objects_completed=1, slides_dropped=1), slide_stride=48),
        Scenario("no slots at all", mp(small[0][2], 5), [], dict(objects_completed=1, slides_dropped=1), max_slides=0),
    ])
    assert 32 + len(small[3][0]) + 24 > 48
    # K: what build_superframe draws
    S["random"] = dict(s=24, num_aus=6, seed=41, body_capacity=256, scenarios=[Scenario("random bodies", [RANDOM] * 72)])
    # L: the chunking stream: objects whose groups cross every super-frame boundary, a label beside them
    ch = [obj(0xB00, image(150, 100), b"first.jpg", 48), obj(0xB01, image(90, 101), b"second.png", 200, hseg=12), obj(0xB02, image(33, 102), b"third", 16)]
    groups = ch[0][2] + ch[1][2] + ch[1][2][:2] + ch[2][2]
    pads = mp(groups, 4, after=synth.dls_fields(LABEL_GROUPS[0] + LABEL_GROUPS[1], 1))
    S["chunks"] = dict(s=8, num_aus=3, seed=42, body_capacity=512, scenarios=[
        Scenario("objects across every boundary", pads, sent((0xB00, ch[0]), (0xB01, ch[1]), (0xB02, ch[2])), dict(groups_repeated=2))])
    # M, N: s = 24, six access units: the directed copies (csrc/wave_copy.hpp; the census of test_pad_device_edges.py counts
    # what they reach).  A segment goes from group offset 9 + (end-user address bytes) to a body offset that is a multiple of
    # the segment size; a completed object's header goes to byte 32 of its slot, its body behind the header.
    mv = [placed_object(0xC00 + i, *a, 110 + i) for i, a in enumerate([
        (1039, 17, 7, 6), (1041, 16, 7, 8), (1009, 62, 7, 8), (41, 8, 7, 0),                         # 16-byte accesses
        (259, 254, 3, 2), (261, 7, 11, 0), (10, 5, 3, 5),                                           # 4-byte accesses
        (70, 9, 1, 3),                      # a byte a lane where source and destination are two bytes apart (mod 4)
        (6, 1, 3, 1), (25, 3, 7, 0)])]      # len < head on either; last, so that what a copy writes beyond them stays in the arena
    S["moves"] = dict(s=24, num_aus=6, seed=43, body_capacity=2048, slots=12, scenarios=[
        Scenario("segments moved by 16-byte words", mp(sum((o[2] for o in mv[:4]), []), 7, per_au=4), sent(*[(0xC00 + i, mv[i]) for i in range(4)]),
                 dict(groups_ok=12, segments_placed=12, slides_written=4), slide_stride=2048),
        Scenario("segments moved by 4-byte words; segments shorter than their head", mp(sum((o[2] for o in mv[4:]), []), 7, per_au=4),
                 sent(*[(0xC00 + i, mv[i]) for i in range(4, 10)]), dict(groups_ok=18, segments_placed=18, slides_written=6), max_slides=6, slide_stride=2048)])
    sl = [sized_object(0xD00 + i, hb, bb, 130 + i) for i, (hb, bb) in enumerate([
        (16, 15), (32, 1009), (48, 1024), (64, 1055),                                               # the body by 16-byte words
        (20, 3), (24, 5), (28, 252), (36, 257), (40, 263),                                          # ... by 4-byte words
        (17, 70), (18, 70)])]                                 # ... a byte a lane, two trips: one and two bytes apart (mod 4)
    S["slotcopies"] = dict(s=24, num_aus=6, seed=44, body_capacity=2048, slots=12, scenarios=[
        Scenario("objects into their slots: %s" % what, mp(sum((o[2] for o in sl[a:b]), []), 7, per_au=4), sent(*[(0xD00 + i, sl[i]) for i in range(a, b)]),
                 dict(groups_ok=2 * (b - a), slides_written=b - a), max_slides=b - a, slide_stride=2048)
        for what, a, b in (("16-byte words", 0, 4), ("4-byte words", 4, 9), ("bytes", 9, 11))])
    # O, P: s = 32, access units laid out by hand: what the kernels fetch of a data stream element (the window `need`)
    lab = lambda text, toggle: [f[0] for f in synth.dls_fields(synth.dls_segments(text, toggle), 5)]
    grp = lambda g: synth.mot_fields([g], 7)[0]
    w0, w1 = obj(0xE00, image(21, 150), b"w0", 64), obj(0xE01, image(75, 151), b"w1", 30)
    assert all(len(g) <= 48 for g in w0[2] + w1[2]) and len(w1[2]) == 4
    l0, l1 = lab(WINDOW_TEXT[0], 0), lab(WINDOW_TEXT[1], 1)
    assert len(l0) == 2 and len(l1) == 2
    counts = [bytes([0x80, 0]), bytes([0x80, 1, 0x20]) + bytes(3), bytes([0x80, 2, 0x20, 0x02]), bytes([0x80, 3, 0x00, 0x20, 0x02]) + bytes(2),
              unit([l0[0]] + grp(w0[2][0]), 253, bytes(5)), unit([l0[1]] + grp(w0[2][1]), 254)]
    escapes = [unit([l1[0]] + grp(w1[2][0]), 255), NO_AUDIO, unit(grp(w1[2][1]), 256, bytes(7)), unit(grp(w1[2][2]), 509, bytes(1)), NO_AUDIO,
               unit([l1[1]] + grp(w1[2][3]), 510)]
    assert [len(u) for u in counts[4:]] == [260, 256] and [len(escapes[i]) for i in (0, 2, 3, 5)] == [258, 266, 513, 513] and escapes[5][1:3] == b"\xff\xff"
    S["window"] = dict(s=32, num_aus=6, seed=45, body_capacity=256, scenarios=[
        Scenario("element counts 0, 1, 2, 3, 253, 254", None, sent((0xE00, w0)), dict(pad_malformed=3, groups_ok=2, aus=6), rows=unit_rows([counts])),
        Scenario("escape bytes 0, 1, 254, 255; a unit that ends with its element of 513 bytes", None, sent((0xE01, w1)),
                 dict(pad_malformed=0, groups_ok=4, aus=6), rows=unit_rows([escapes]))])
    # the stale row: slot a of one super-frame holds a valid unit (a label segment and a data group, whole), slot a of the next
    # one begins with the same bytes and is (i) a byte short of its count, (ii) cut behind the count 255, (iii) without the
    # element's tag; a = 0 and the last unit visited -- the seventh, of nine claimed, or the sixth with a seventh claimed
    stale = []
    for i, (what, n, seven, spoil_unit, malformed) in enumerate([
            ("a byte too short for its count", 100, True, lambda v: (v[:-1], v[-1:]), 2),
            ("the count 255 and no escape byte", 300, True, lambda v: v[:2], 2),
            ("no element tag in front of the same bytes", 100, True, lambda v: b"\x21" + v[1:], 0),
            ("a byte too short, six units and a seventh claimed", 120, False, lambda v: (v[:-1], v[-1:]), 2)]):
        o, text = obj(0xF00 + i, image(30, 160 + i), b"st%d" % i, 64), lab(STALE_TEXT[i], i & 1)
        first, last = unit([text[0]] + grp(o[2][0]), n), unit([text[1]] + grp(o[2][1]), n)
        assert len(text) == 2 and len(o[2]) == 2 and (n < 255 or first[1] == 255)
        quiet = [NO_AUDIO] * (5 if seven else 4)
        stale.append(Scenario("a stale row: " + what, None, sent((0xF00 + i, o)),
                              dict(pad_malformed=malformed, groups_ok=2, slides_written=1, aus=14, aus_lost=0 if seven else 2),
                              rows=unit_rows([[first] + quiet + [last], [spoil_unit(first)] + quiet + [spoil_unit(last)]], claim=9 if seven else 7)))
    S["stale"] = dict(s=32, num_aus=6, seed=46, body_capacity=256, scenarios=stale)
    return S


WINDOW_TEXT = [b"counts below the escape", b"and the escape byte itself"]
STALE_TEXT = [b"stale row, one byte short", b"stale row, cut at the count", b"stale row, no element tag", b"stale row, the sixth unit"]
LABEL_TEXT = [b"Now: a slide beside this label", b"and another one"]
LABEL_GROUPS = [synth.dls_segments(LABEL_TEXT[0], 0), synth.dls_segments(LABEL_TEXT[1], 1)]
STREAMS = _streams()


@pytest.fixture(scope="module")
def built_streams(built):
    """name -> dict(s, body_capacity, data, status, bounds: [(scenario, first super-frame, end)])"""
    out = {}
    for name, spec in STREAMS.items():
        datas, stats, bounds, at = [], [], [], 0
        for k, sc in enumerate(spec["scenarios"]):
            d, st = sc.rows(spec["s"]) if sc.rows else superframes(spec["seed"] * 100 + k, spec["s"], spec["num_aus"], sc.pads)
            if sc.damage:
                sc.damage(st)
            datas.append(d); stats.append(st)
            bounds.append((sc, at, at + len(d)))
            at += len(d)
        out[name] = dict(s=spec["s"], body_capacity=spec["body_capacity"], data=np.concatenate(datas), status=np.concatenate(stats), bounds=bounds,
                         slots=spec.get("slots"))
        assert at <= 16, (name, at)
    return out


# ------------------------------------------------------------------------------------------------ one call, on any memory
class HostMemory:
    def load(self, img):
        raw = np.empty(img.size + 256, np.uint8)
        off = -raw.ctypes.data % 256
        self.buf = raw[off:off + img.size]
        self.buf[:] = img
        return self.buf.ctypes.data

    def run(self, entries):
        dabgpu.mot_slides_host(entries)

    def read(self):
        return self.buf.copy()


class DeviceMemory:
    def __init__(self, ctx):
        self.ctx = ctx

    def load(self, img):
        import torch
        self.t = torch.from_numpy(img).cuda()
        return self.t.data_ptr()

    def run(self, entries):
        self.ctx.mot_slides_dev(entries)
        self.ctx.sync()

    def read(self):
        self.ctx.sync()
        return self.t.cpu().numpy()


def stride_of(sp):
    return sp.get("slide_stride") or 1024


def call(mem, specs, mutate=None, refused=False):
    """One call on buffers laid out in one allocation, every region between sentinel bytes.  specs: dicts {s, data, status, n,
    max_sf, state (bytes or None = NULL), arena (bytes or None = sentinel bytes), body_capacity, max_slides, slide_stride,
    stride, data_off (the data rows begin that many bytes, below 16, off their 256-byte boundary)}.  After the call nothing but state-out, arena, result and the slots' written bytes may have changed (nothing at
    all for a refused call).  -> per entry dict(slides [(record, header, body)], result, state, arena)"""
    size, lay = 0, []

    def take(n):
        nonlocal size
        off = (size + GAP + 255) // 256 * 256
        size = off + n
        return off

    nb = dabgpu.mot_state_bytes()
    for sp in specs:
        rows, stride = len(sp["data"]), sp.get("stride", 110 * sp["s"])
        ab = dabgpu.mot_arena_bytes(sp["body_capacity"])
        assert ab == M.arena_bytes(sp["body_capacity"])
        assert 0 <= sp.get("data_off", 0) < 16
        lay.append(dict(data=take(max(rows, 1) * stride + 16) + sp.get("data_off", 0), status=take(max(rows, 1) * 64), follow=take(32),
                        sin=take(nb) if sp.get("state") is not None else None, sout=take(nb), arena=take(ab), ab=ab,
                        slides=take(max(sp.get("max_slides", 4), 1) * stride_of(sp)), result=take(128)))
    img = np.full(size + GAP, FILL, np.uint8)
    for sp, L in zip(specs, lay):
        stride = sp.get("stride", 110 * sp["s"])
        for k, row in enumerate(sp["data"]):
            img[L["data"] + k * stride:L["data"] + k * stride + row.size] = row
        img[L["status"]:L["status"] + 64 * len(sp["data"])] = np.asarray(sp["status"]).view(np.uint8).reshape(-1)
        fr = np.zeros(1, dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)
        fr["n_superframes"], fr["phase"], fr["synced"] = sp["n"], 0, 1
        img[L["follow"]:L["follow"] + 32] = fr.view(np.uint8)
        if L["sin"] is not None:
            img[L["sin"]:L["sin"] + nb] = np.frombuffer(bytes(sp["state"]), np.uint8)
        if sp.get("arena") is not None:
            img[L["arena"]:L["arena"] + L["ab"]] = sp["arena"]
    base = mem.load(img)
    assert base % 256 == 0
    # (what the census of copy classes in test_pad_device_edges.py rests on: arena and slots on 16-byte boundaries)
    assert all((base + L["arena"]) % 16 == 0 and (base + L["slides"]) % 16 == 0 and stride_of(sp) % 16 == 0 for sp, L in zip(specs, lay))
    entries = [dabgpu.MotEntry(base + L["data"], sp.get("stride", 110 * sp["s"]), base + L["status"], base + L["follow"], 8 * sp["s"],
                               sp.get("max_sf", len(sp["data"])), base + L["sin"] if L["sin"] is not None else None, base + L["sout"],
                               base + L["arena"], L["ab"], base + L["slides"], stride_of(sp), sp.get("max_slides", 4), 0, base + L["result"])
               for sp, L in zip(specs, lay)]
    if mutate:
        mutate(entries)
    if refused:
        with pytest.raises(dabgpu.DabGpuError) as err:
            mem.run(entries)
        assert err.value.status == ARG
        assert (mem.read() == img).all(), "a refused call wrote"
        return None
    mem.run(entries)
    after = mem.read()
    out, untouched = [], np.ones(after.size, bool)
    for sp, L in zip(specs, lay):
        for key, n in (("sout", nb), ("arena", L["ab"]), ("result", 128)):
            untouched[L[key]:L[key] + n] = False
        res = after[L["result"]:L["result"] + 128].copy().view(dabgpu.MOT_RESULT_DTYPE)
        written = int(res["slides_written"][0])
        assert 0 <= written <= sp.get("max_slides", 4)
        slides = []
        for k in range(written):
            at = L["slides"] + k * stride_of(sp)
            rec = after[at:at + 32].copy().view(dabgpu.MOT_SLIDE_DTYPE)
            hb, bb = int(rec["header_bytes"][0]), int(rec["body_bytes"][0])
            assert 0 <= hb and 0 <= bb and 32 + hb + bb <= stride_of(sp), rec
            untouched[at:at + 32 + hb + bb] = False
            slides.append((rec, after[at + 32:at + 32 + hb].tobytes(), after[at + 32 + hb:at + 32 + hb + bb].tobytes()))
        out.append(dict(slides=slides, result=res, state=after[L["sout"]:L["sout"] + nb].copy(), arena=after[L["arena"]:L["arena"] + L["ab"]].copy()))
    assert (after[untouched] == img[untouched]).all(), "bytes outside the outputs changed"
    return out


def same(got, want):
    """got: an entry of call(); want: (slides, result record) of the reference: byte for byte"""
    ws, wr = want
    return (got["result"].tobytes() == wr.tobytes() and len(got["slides"]) == len(ws) and
            all(g[0].tobytes() == w[0].tobytes() and g[1] == w[1] and g[2] == w[2] for g, w in zip(got["slides"], ws)))


def explain(got, want):
    return "\n got  %s %s\n want %s %s" % ([g[0] for g in got["slides"]], got["result"], [w[0] for w in want[0]], want[1])


def spec_of(st, a, b, sc=None, **kw):
    sp = dict(s=st["s"], data=st["data"][a:b], status=st["status"][a:b], n=b - a, body_capacity=st["body_capacity"])
    if sc is not None:
        sp.update(max_slides=sc.max_slides, slide_stride=sc.slide_stride)
    sp.update(kw)
    return sp


def ref_call(rx, sp, n=None):
    return rx.call(sp["data"], sp["status"], sp["n"] if n is None else n, sp["s"], sp.get("max_slides", 4), stride_of(sp))


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_records_and_sizes(built, tmp_path):
    L = dabgpu.lib()
    for name in ("dabgpu_mot_state_bytes", "dabgpu_mot_arena_bytes", "dabgpu_mot_slides_dev", "dabgpu_mot_slides_host", "dabgpu_mot_header_parse"):
        assert name in dabgpu.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.dabgpu_abi_version() == 6 == dabgpu.ABI_VERSION
    assert dabgpu.MOT_RESULT_DTYPE.itemsize == 128 == M.RESULT_DTYPE.itemsize and dabgpu.MOT_RESULT_DTYPE.names == M.RESULT_DTYPE.names
    assert dabgpu.MOT_SLIDE_DTYPE.itemsize == 32 == M.SLIDE_DTYPE.itemsize and dabgpu.MOT_SLIDE_DTYPE.names == M.SLIDE_DTYPE.names
    assert dabgpu.mot_state_bytes() % 16 == 0 and hasattr(dabgpu.Context, "mot_slides_dev")
    assert dabgpu.mot_arena_bytes(0) == M.arena_bytes(0) and dabgpu.mot_arena_bytes(1) == M.arena_bytes(0) + 16
    assert dabgpu.mot_arena_bytes(256 * 8191) > 0 and dabgpu.mot_arena_bytes(256 * 8191 + 1) == 0
    # the binding's structures and the records against the header, as the C compiler lays them out
    structs = [("dabgpu_mot_entry", dabgpu.MotEntry), ("dabgpu_mot_header", dabgpu.MotHeader), ("dabgpu_mot_text", dabgpu.MotText)]
    records = [("dabgpu_mot_slide", dabgpu.MOT_SLIDE_DTYPE), ("dabgpu_mot_result", dabgpu.MOT_RESULT_DTYPE)]
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


def spoil(field, value, at=-1):
    def f(entries):
        setattr(entries[at], field, value(entries[at]) if callable(value) else value)
    return f


#: each refused with DABGPU_ERR_ARG, the bad entry LAST in the table: nothing of the good ones before it is written
BAD_ENTRIES = [spoil("bitrate_kbps", 12), spoil("bitrate_kbps", 0), spoil("bitrate_kbps", 520), spoil("data_stride", 879),
               spoil("max_superframes", -1), spoil("d_data", None), spoil("d_status", None), spoil("d_follow", None),
               spoil("d_state_out", None), spoil("d_arena", None), spoil("d_slides", None), spoil("d_result", None),
               spoil("d_state_in", lambda e: e.d_state_in + 8), spoil("d_state_out", lambda e: e.d_state_out + 4),
               spoil("d_state_out", lambda e: e.d_state_in), spoil("d_state_out", lambda e: e.d_state_in + 16),
               spoil("d_state_out", lambda e: e.d_state_in - 16), spoil("d_arena", lambda e: e.d_arena + 8),
               spoil("d_slides", lambda e: e.d_slides + 4), spoil("d_result", lambda e: e.d_result + 1),
               spoil("d_status", lambda e: e.d_status + 2), spoil("d_follow", lambda e: e.d_follow + 2),
               spoil("arena_bytes", lambda e: dabgpu.mot_arena_bytes(0) - 16), spoil("arena_bytes", 0), spoil("max_slides", -1),
               spoil("slide_stride", 16), spoil("slide_stride", 1000), spoil("slide_stride", 1 << 31), spoil("max_slides", 1 << 21)]


def refusal_specs(built_streams):
    st = built_streams["bodies"]
    zero = np.zeros(dabgpu.mot_state_bytes(), np.uint8)
    return [spec_of(st, 0, 2, state=zero) for _ in range(3)]


def test_refusals_that_need_no_device(built_streams):
    L = dabgpu.lib()
    specs = refusal_specs(built_streams)
    for m in BAD_ENTRIES:
        call(HostMemory(), specs, mutate=m, refused=True)
    good = (dabgpu.MotEntry * 1)(dabgpu.MotEntry(0x10000, 880, 0x20000, 0x30000, 64, 2, None, 0x40000, 0x50000, dabgpu.mot_arena_bytes(64),
                                                 0x60000, 1024, 1, 0, 0x70000))
    assert L.dabgpu_mot_slides_host(None, 1) == ARG and L.dabgpu_mot_slides_host(good, -1) == ARG
    assert L.dabgpu_mot_slides_host(None, 0) == 0
    assert L.dabgpu_mot_slides_dev(None, good, 1, None) == ARG      # no context: refused before anything is looked for
    got = call(HostMemory(), specs)                                  # ... and the unspoilt table goes through
    assert all(int(r["result"]["aus"][0]) == 6 and len(r["slides"]) == 2 for r in got)
    # d_slides may be NULL where there are no slots
    call(HostMemory(), [dict(specs[0], max_slides=0)], mutate=spoil("d_slides", None))


@pytest.mark.parametrize("name", list(STREAMS))
def test_host_equals_the_reference_scenario_by_scenario(built_streams, name):
    """one call per scenario, state and arena handed on: slides and counters equal the reference's; the reference itself
    reports what the scenario is about, and the objects that were sent"""
    st = built_streams[name]
    rx, state, arena = M.Receiver(st["body_capacity"]), None, None
    for sc, a, b in st["bounds"]:
        sp = spec_of(st, a, b, sc, state=state, arena=arena)
        want = ref_call(rx, sp)
        got = call(HostMemory(), [sp])[0]
        assert same(got, want), sc.name + explain(got, want)
        state, arena = got["state"], got["arena"]
        assert [(int(r["transport_id"][0]), h, bd) for r, h, bd in want[0]] == sc.slides, sc.name
        assert all(int(r["content_type"][0]) == 2 and int(r["content_subtype"][0]) == 1 for r, _h, _b in want[0])
        for key, value in sc.counts.items():
            assert int(want[1][key][0]) == value, (sc.name, key, want[1])


def test_scenarios_cover_what_they_should():
    names = [sc.name for spec in STREAMS.values() for sc in spec["scenarios"]]
    assert len(names) == len(set(names)) >= 40
    assert {(v["s"], v["num_aus"]) for v in STREAMS.values()} >= {(8, 3), (24, 6), (8, 4), (8, 6)}
    assert synth.dgli(0x3FFF)[:2] == b"\x3f\xff" and P.crc_ccitt(synth.dgli(300)[:2]) == int.from_bytes(synth.dgli(300)[2:], "big")
    g = synth.mot_group(4, 0x1234, 5, True, b"abc", extension=7, end_user=b"\x09")
    assert g[0] == 0xF4 and g[2:4] == b"\x00\x07" and g[4:6] == b"\x80\x05" and g[6] == 0x13 and g[7:9] == b"\x12\x34" and g[9] == 9
    assert g[10:12] == b"\x00\x03" and g[12:15] == b"abc" and len(g) == 17
    h = synth.mot_header(0x1234567, 2, 3, [synth.mot_param(0x0C, b"\xf0x")])
    assert int.from_bytes(h[:7], "big") == (0x1234567 << 28) | (11 << 15) | (2 << 9) | 3 and h[7:] == b"\xcc\x02\xf0x"


def test_label_beside_the_slide_is_what_the_label_call_gives(built_streams):
    """the layouts stream through the label call: the labels that travel beside the slides, exactly"""
    import test_pad_labels as T
    st = built_streams["layouts"]
    want = P.Receiver().call(st["data"], st["status"], len(st["data"]), st["s"])
    got = T.call(T.HostMemory(), [dict(s=st["s"], data=st["data"], status=st["status"], n=len(st["data"]))])[0]
    assert T.same(got, want) and T.text_of(got[0]) == LABEL_TEXT[1] and int(got[1]["labels_completed"][0]) == 2
    first = P.Receiver().call(st["data"][:st["bounds"][1][2]], st["status"], st["bounds"][1][2], st["s"])
    assert T.text_of(first[0]) == LABEL_TEXT[0]


def wide(st):
    return 8192 + 128 if st["body_capacity"] > 4096 else 2048


def run_cut(mem_of, st, cuts, max_slides=12):
    """the stream in calls that end at `cuts` (and its end), state and arena handed on -> (slides of all calls, summed
    counters, last state, last arena, per call (slides, result))"""
    state, arena, at, slides, results, calls = None, None, 0, [], [], []
    n = len(st["data"])
    for end in list(cuts) + [n]:
        rows = (at, end) if end > at else (0, 1)                     # a call of no super-frames keeps a row: d_follow says 0
        sp = spec_of(st, rows[0], rows[1], state=state, arena=arena, max_slides=max_slides, slide_stride=wide(st))
        sp["n"] = end - at
        r = call(mem_of(), [sp])[0]
        state, arena, at = r["state"], r["arena"], end
        slides += r["slides"]
        results.append(r["result"])
        calls.append(r)
    return slides, M.total(results), state, arena, calls


def strip(slides):
    """slides without where in their call they completed"""
    return [(int(r["transport_id"][0]), int(r["content_type"][0]), int(r["content_subtype"][0]), h, b) for r, h, b in slides]


@pytest.mark.parametrize("name", list(STREAMS))
def test_cut_at_every_superframe_boundary(built_streams, name):
    """each stream in one call, and cut into two calls at EVERY super-frame boundary with state and arena carried: the
    slides, the summed counters and the state record equal the uncut run's; so does one call per super-frame"""
    st = built_streams[name]
    n = len(st["data"])
    whole = run_cut(HostMemory, st, [])
    rx = M.Receiver(st["body_capacity"])
    ref = rx.call(st["data"], st["status"], n, st["s"], 12, wide(st))
    assert strip(whole[0]) == strip(ref[0]) and whole[1] == M.total([ref[1]])
    for cuts in [[k] for k in range(0, n + 1)] + [list(range(1, n))]:
        got = run_cut(HostMemory, st, cuts)
        assert strip(got[0]) == strip(whole[0]) and got[1] == whole[1], (name, cuts)
        assert got[2].tobytes() == whole[2].tobytes(), (name, cuts)


def test_a_foreign_state_record_is_a_fresh_start(built_streams):
    st = built_streams["bodies"]
    rng = np.random.default_rng(7)
    sp = spec_of(st, 0, len(st["data"]))
    want = ref_call(M.Receiver(st["body_capacity"]), sp)
    for k in range(40):
        state = rng.integers(0, 256, dabgpu.mot_state_bytes(), dtype=np.uint8)
        if k % 2:                                                     # nearly ours: a record of this library's with one byte changed
            state = call(HostMemory(), [dict(spec_of(st, 0, 3), n=2)])[0]["state"]
            state[rng.integers(0, state.size)] ^= 1 << rng.integers(0, 8)
        got = call(HostMemory(), [dict(sp, state=state)])[0]                # (whatever it holds: nothing outside the outputs is written)
        if k % 2 == 0:
            assert same(got, want), k
    # a record written for another arena size is a fresh start, too
    other = call(HostMemory(), [dict(spec_of(st, 0, 3), n=2, body_capacity=64)])[0]["state"]
    assert same(call(HostMemory(), [dict(sp, state=other)])[0], want)


# ---- the header parser
NAME = "Ωmega – cover.jpg".encode("utf-8")
FULL_PARAMS = [synth.mot_param(0x0C, bytes([15 << 4]) + NAME), synth.mot_param(0x05, synth.mot_time()),
               synth.mot_param(0x04, synth.mot_time(60000, 13, 37)), synth.mot_param(0x25, bytes([3, 17])),
               synth.mot_param(0x26, b"Album art"), synth.mot_param(0x27, b"http://example.org/" + b"x" * 150),
               synth.mot_param(0x28, b"http://example.org/a.jpg", pli=3, long_length=True), synth.mot_param(0x10),
               synth.mot_param(0x11, b"\x01"), synth.mot_param(0x12, bytes(4)), synth.mot_param(0x3F, bytes(9)),
               synth.mot_param(0x05, synth.mot_time(60001, 1, 2) + b"\x00\x00", pli=3)]
FULL_HEADER = synth.mot_header(12345, 2, 3, FULL_PARAMS)


def parse(h):
    try:
        return dabgpu.mot_header_parse(h)
    except dabgpu.DabGpuError as e:
        return {ARG: None, CAPACITY: "capacity"}[e.status]


def test_header_parse_every_parameter(built):
    want = M.parse_header(FULL_HEADER)
    assert want["name"] == NAME and want["name_charset"] == 15 and want["expire"] == (1 << 31) | (60000 << 14) | (13 << 6) | 37
    assert want["trigger"] == (1 << 31) | (60001 << 14) | (1 << 6) | 2 and want["category_id"] == 3 and want["slide_id"] == 17
    assert want["category_title"] == b"Album art" and len(want["click_through_url"]) == 169 and want["alternative_location_url"] == b"http://example.org/a.jpg"
    assert want["n_params"] == 12 and want["n_unknown"] == 4 and (want["body_size"], want["content_type"], want["content_subtype"]) == (12345, 2, 3)
    assert parse(FULL_HEADER) == want
    core = synth.mot_header(0, 2, 1)
    assert parse(core) == M.parse_header(core) and parse(core)["name"] is None and parse(core)["trigger"] is None
    now = synth.slide_header(5, b"now.png", subtype=3)
    assert parse(now) == M.parse_header(now) and parse(now)["trigger"] == "now" and parse(now)["content_subtype"] == 3
    for data in (b"", b"\xf0", bytes([0x40]) + b"y" * 255, bytes([0x40]) + b"y" * 256):
        h = synth.mot_header(1, 2, 1, [synth.mot_param(0x0C, data, pli=3)])
        assert parse(h) == M.parse_header(h), data[:4]
    assert parse(synth.mot_header(1, 2, 1, [synth.mot_param(0x0C, b"", pli=3)])) is None
    assert parse(synth.mot_header(1, 2, 1, [synth.mot_param(0x0C, bytes([0x40]) + b"y" * 256)])) == "capacity"
    for params in ([synth.mot_param(0x05, b"\x80")], [synth.mot_param(0x04, b"\x80\x00\x00", pli=3)], [synth.mot_param(0x25, b"\x01")]):
        h = synth.mot_header(1, 2, 1, params)
        assert parse(h) is None and M.parse_header(h) is None
    L = dabgpu.lib()
    raw = np.frombuffer(FULL_HEADER, np.uint8)
    assert L.dabgpu_mot_header_parse(raw.ctypes.data, raw.size, None) == ARG and L.dabgpu_mot_header_parse(None, raw.size, C.byref(dabgpu.MotHeader())) == ARG


def test_header_parse_refuses_every_truncation(built):
    """a valid header cut at every byte, as it is and with its header_size made to fit: refused wherever the reference
    refuses, nothing written"""
    L = dabgpu.lib()
    refused = 0
    for n in range(len(FULL_HEADER)):
        cut = FULL_HEADER[:n]
        assert parse(cut) is None and M.parse_header(cut) is None, n
        fitted = synth.mot_header(12345, 2, 3, [FULL_HEADER[7:n]])[:max(n, 7)] if n >= 7 else cut
        want = M.parse_header(fitted)
        refused += want is None
        out = dabgpu.MotHeader()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        raw = np.frombuffer(fitted + b"\x00", np.uint8)
        rc = L.dabgpu_mot_header_parse(raw.ctypes.data, len(fitted), C.byref(out))
        assert (rc == 0) == (want is not None), n
        if want is None:
            assert bytes(out) == b"\x5a" * C.sizeof(out), n
        else:
            assert parse(fitted) == want, n
    assert refused > len(FULL_HEADER) * 3 // 4


# ---- device code, sanitizers
def test_new_kernel_neither_spills_nor_uses_scratch(built, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the device assembly cannot be checked")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    out = tmp_path / "mot_kernels.s"
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "mot_kernels.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    md = kernel_metadata(out.read_text())
    kernels = [v for k, v in md.items() if "mot_slides_kernel" in k]
    assert len(kernels) == 1 and len(md) == 1
    v = kernels[0]
    print("mot_slides_kernel: vgprs %s, sgprs %s, LDS %s bytes" % (v.get("vgpr_count"), v.get("sgpr_count"), v.get("group_segment_fixed_size")))
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v


def test_walk_fuzz_under_sanitizers(tmp_path):
    """tests/mot_walk_fuzz.cpp: walks over random and mutated-valid access units, each at the end of an exactly sized heap
    block, the arena and the slots exactly sized too, the copy orders executed with their bounds asserted; built with the
    host compiler under AddressSanitizer and UBSan and run as a child process"""
    exe = str(tmp_path / "mot_walk_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mot_walk_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "150000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "walks=150000" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = dict(kv.split("=") for kv in r.stdout.split())
    print(r.stdout)
    assert int(got["slides"]) > 0 and int(got["malformed"]) > 0 and int(got["lost"]) > 0, r.stdout


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


def ragged_specs(built_streams):
    specs = []
    for e, (name, st) in enumerate(built_streams.items()):
        n = len(st["data"])
        ff = np.full((2, 110 * st["s"]), 0xFF, np.uint8)
        ffs = np.full(2 * 64, 0xFF, np.uint8).view(P.STATUS_DTYPE)
        specs.append(dict(s=st["s"], data=np.concatenate([st["data"], ff]), status=np.concatenate([st["status"], ffs]), n=n, body_capacity=st["body_capacity"],
                          stride=110 * st["s"] + [0, 2, 16][e % 3], max_slides=st["slots"] or [8, 2, 5][e % 3], slide_stride=8192 + 128 if st["body_capacity"] > 4096 else 2048))
    return specs


@pytest.mark.gpu
def test_gpu_every_case_in_one_ragged_call(pctx, built_streams):
    """all streams in ONE call: bit rates 64 and 192, n_superframes read from the device's follow records, two rows of 0xFF
    behind every stream, different slot counts: slides, counters, state record and arena equal the reference and the host call"""
    specs = ragged_specs(built_streams)
    wants = [ref_call(M.Receiver(sp["body_capacity"]), sp) for sp in specs]
    got = call(DeviceMemory(pctx), specs)
    host = call(HostMemory(), specs)
    for name, g, h, w in zip(built_streams, got, host, wants):
        assert same(g, w), name + explain(g, w)
        assert same(h, w), name
        assert g["state"].tobytes() == h["state"].tobytes() and (g["arena"] == h["arena"]).all(), name
    assert sum(len(g["slides"]) for g in got) >= 30 and sum(int(g["result"]["slides_dropped"][0]) for g in got) >= 5


@pytest.mark.gpu
def test_gpu_three_cuts_with_the_state_on_the_device(pctx, built_streams):
    """every stream in three calls, state records swapped and the arena in place on the device, all streams in each call:
    slides and summed counters equal the uncut host run's, the last state record too"""
    import torch
    names = list(built_streams)
    nb = dabgpu.mot_state_bytes()
    keep, per, totals = [], {n: [] for n in names}, {n: [] for n in names}
    bufs = {}
    for name in names:
        st = built_streams[name]
        n, stride = len(st["data"]), 8192 + 128 if st["body_capacity"] > 4096 else 2048
        bufs[name] = dict(data=torch.from_numpy(st["data"]).cuda(), status=torch.from_numpy(st["status"].view(np.uint8).reshape(n, 64).copy()).cuda(),
                          follow=torch.zeros((3, 32), dtype=torch.uint8), states=torch.zeros((2, nb), dtype=torch.uint8, device="cuda"),
                          arena=torch.full((dabgpu.mot_arena_bytes(st["body_capacity"]),), FILL, dtype=torch.uint8, device="cuda"),
                          slides=torch.full((3, 8, stride), FILL, dtype=torch.uint8, device="cuda"), results=torch.zeros((3, 128), dtype=torch.uint8, device="cuda"),
                          cuts=[0, n // 3, 2 * n // 3, n], stride=stride)
        fr = np.zeros(3, dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)
        fr["n_superframes"] = np.diff(bufs[name]["cuts"])
        bufs[name]["follow"] = torch.from_numpy(fr.view(np.uint8).reshape(3, 32).copy()).cuda()
    for k in range(3):
        entries = []
        for name in names:
            b, st = bufs[name], built_streams[name]
            row = min(b["cuts"][k], len(st["data"]) - 1)
            entries.append(dabgpu.MotEntry(b["data"][row].data_ptr(), 110 * st["s"], b["status"][row].data_ptr(), b["follow"][k].data_ptr(), 8 * st["s"],
                                           len(st["data"]) - row, b["states"][k & 1].data_ptr() if k else None, b["states"][~k & 1].data_ptr(),
                                           b["arena"].data_ptr(), b["arena"].numel(), b["slides"][k].data_ptr(), b["stride"], 8, 0, b["results"][k].data_ptr()))
        pctx.mot_slides_dev(entries)                                 # nothing waits between the calls
    pctx.sync()
    for name in names:
        b, st = bufs[name], built_streams[name]
        whole = run_cut(HostMemory, st, [])
        res = b["results"].cpu().numpy().view(dabgpu.MOT_RESULT_DTYPE).reshape(3)
        raw = b["slides"].cpu().numpy()
        slides = []
        for k in range(3):
            for j in range(int(res[k]["slides_written"])):
                rec = raw[k, j, :32].copy().view(dabgpu.MOT_SLIDE_DTYPE)
                hb, bb = int(rec["header_bytes"][0]), int(rec["body_bytes"][0])
                slides.append((rec, raw[k, j, 32:32 + hb].tobytes(), raw[k, j, 32 + hb:32 + hb + bb].tobytes()))
                assert (raw[k, j, 32 + hb + bb:] == FILL).all()
            assert (raw[k, int(res[k]["slides_written"]):] == FILL).all()
        assert strip(slides) == strip(whole[0]), name
        assert M.total([res[k:k + 1] for k in range(3)]) == whole[1], name
        assert b["states"][1].cpu().numpy().tobytes() == whole[2].tobytes(), name


@pytest.mark.gpu
def test_gpu_refused_calls_leave_every_output_alone(pctx, built_streams):
    specs = refusal_specs(built_streams)
    for m in BAD_ENTRIES:
        call(DeviceMemory(pctx), specs, mutate=m, refused=True)
    pctx.mot_slides_dev([])                                          # nothing to do is not an error
    got = call(DeviceMemory(pctx), specs)
    assert all(len(r["slides"]) == 2 for r in got)


# ---- end to end
E2E_SERVICES = [("Radio One", 0xC221, 3, 0, 3, 64, 0), ("Jazz 24", 0xC222, 7, 0, 2, 32, 48)]       # s = 8 and s = 4
E2E_LABELS = ["Now: Ω Quartet – Blue in Green".encode("utf-8"), "Nachrichten um 12".encode("utf-8")]
E2E_NAMES = [b"cover-0817.jpg", b"news.png"]
E2E_SEED = 1                                                          # (a cycle of twelve access units has room for slide and label)
E2E_OBJECTS = [obj(0x1000 + j, image(300 - 9 * j, 200 + j), E2E_NAMES[j], 128) for j in range(2)]


def e2e_au_sizes(seed):
    """the access unit sizes ServiceEnsemble(seed, E2E_SERVICES, n_frames=5) will draw (its draws do not depend on the bodies)"""
    rng = np.random.default_rng(seed)
    rng.integers(0, 2, size=(20, synth.NB_CIF_BITS), dtype=np.uint8)
    return [[[len(a) for a in synth.build_superframe(rng, svc[5], dac_rate=1, sbr=1, channel_mode=1, ps=0)[2]] for _q in range(4)] for svc in E2E_SERVICES]


def e2e_bodies(seed=E2E_SEED):
    sizes = e2e_au_sizes(seed)
    bodies, left = [], 0
    for j in range(2):
        flat = [n for q in sizes[j] for n in q]
        pads, rest = synth.pack_pads(flat, E2E_OBJECTS[j][2], synth.dls_segments(E2E_LABELS[j], j))
        left += rest
        bodies.append([[synth.au_body(p) if p is not None else NO_PAD for p in pads[3 * q:3 * q + 3]] for q in range(4)])
    return bodies, left


def test_end_to_end_multiplex_carries_both_slides_and_labels(built):
    """what the GPU test will receive, through the reference receivers on the transmitted super-frames"""
    bodies, left = e2e_bodies()
    assert left == 0, "the cycle has no room for slide and label"
    ens = synth.ServiceEnsemble(E2E_SEED, E2E_SERVICES, n_frames=5, extras=False, bodies=bodies)
    assert [[[len(a) for a in q] for q in sv] for sv in ens.aus] == e2e_au_sizes(E2E_SEED)
    for n, svc in enumerate(E2E_SERVICES):
        s = svc[5] // 8
        data = np.stack([sf[:110 * s] for sf in ens.superframes[n]])
        status = np.zeros(4, P.STATUS_DTYPE)
        status["firecode_ok"], status["num_aus"], status["au_crc_mask"] = 1, 3, 7
        for q in range(4):
            status[q]["au_start"][:4] = [6] + [6 + sum(len(a) for a in ens.aus[n][q][:k + 1]) for k in range(3)]
        lab, res = P.Receiver().call(data, status, 4, s)
        assert bytes(lab["text"][0][:int(lab["length"][0])]) == E2E_LABELS[n] and int(res["pad_malformed"][0]) == 0, (n, res)
        slides, counts = M.Receiver(512).call(data, status, 4, s, 2, 1024)
        assert strip(slides) == [(0x1000 + n, 2, 1, E2E_OBJECTS[n][0], E2E_OBJECTS[n][1])], (n, counts)
        assert dabgpu.mot_header_parse(slides[0][1])["name"] == E2E_NAMES[n]


@pytest.mark.gpu
def test_gpu_end_to_end_iq_to_slides_and_labels(pctx):
    """IQ of a multiplex whose two DAB+ services (64 and 32 kbit/s) each carry a slide and a label in the same PAD -> front
    end -> FIC pass -> decode_ensembles_dev -> dabplus_follow_dev -> mot_slides_dev and pad_labels_dev on the same stream,
    three calls of 16 frames, the records swapped, the arena in place: both slides and both labels as sent, each slide once"""
    import torch
    dev = torch.device("cuda", 0)
    fps, n_calls, L, FB = 16, 3, 76 * 2552, dabgpu.NB_FRAME_BITS
    ens = synth.ServiceEnsemble(E2E_SEED, E2E_SERVICES, n_frames=5, extras=False, bodies=e2e_bodies()[0])
    tx = ens.iq()
    rng = np.random.default_rng(12)
    c = pctx
    c.streams_reset(1)
    plans = None
    n_cifs, max_sf, nb, mb = 4 * fps, (4 * fps + 4) // 5, dabgpu.pad_state_bytes(), dabgpu.mot_state_bytes()
    labels = torch.zeros((2, 144), dtype=torch.uint8, device=dev)
    slots = torch.full((n_calls, 2, 2, 1024), FILL, dtype=torch.uint8, device=dev)
    results = torch.zeros((n_calls, 2, 128), dtype=torch.uint8, device=dev)
    for call_no in range(n_calls):
        idx = (np.arange(fps) + call_no * fps) % 5
        rx = synth.channel(tx[idx].ravel(), snr_db=20.0, rng=rng).reshape(fps, -1)
        d_iq = torch.from_numpy(np.ascontiguousarray(rx[:, synth.NB_NULL:synth.NB_NULL + L]).astype(np.complex64)).to(dev)
        d_soft = torch.zeros((fps, FB), dtype=torch.int8, device=dev)
        c.ofdm_demod_streams_dev(d_iq.data_ptr(), L, 1, fps, 0.9, d_soft.data_ptr(), None, None)
        fib = torch.zeros((fps, 12, 32), dtype=torch.uint8, device=dev)
        ok = torch.zeros((fps, 12), dtype=torch.uint8, device=dev)
        if plans is None:
            c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), [[]], None, None, None, None)
            c.sync()
            fib_h, ok_h = fib.cpu().numpy(), ok.cpu().numpy()
            assert ok_h.all()
            plans = [dabgpu.fig_subchannels(fib_h, ok_h)]
            assert [sc.bitrate_kbps for sc in plans[0]] == [64, 32]
            hist = [[[torch.zeros((15, sc.length * 64), dtype=torch.int8, device=dev) for sc in plans[0]]] for _ in range(2)]
            carry = [[torch.zeros(dabgpu.dabplus_carry_bytes(sc.bitrate_kbps), dtype=torch.uint8, device=dev) for sc in plans[0]] for _ in range(2)]
            state = [[torch.zeros(nb, dtype=torch.uint8, device=dev) for _sc in plans[0]] for _ in range(2)]
            mstate = [[torch.zeros(mb, dtype=torch.uint8, device=dev) for _sc in plans[0]] for _ in range(2)]
            arenas = [torch.zeros(dabgpu.mot_arena_bytes(512), dtype=torch.uint8, device=dev) for _sc in plans[0]]
        outs = [[torch.zeros((n_cifs, sc.bitrate_kbps * 3), dtype=torch.uint8, device=dev) for sc in plans[0]]]
        ptrs = lambda lsts: [[x.data_ptr() for x in lst] for lst in lsts]
        c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), plans, ptrs(hist[0]) if call_no else None,
                               ptrs(hist[1]), ptrs(outs), None)
        follow, pads, mots, keep = [], [], [], []
        for j, sc in enumerate(plans[0]):
            br = sc.bitrate_kbps
            data = torch.zeros((max_sf, 110 * br // 8), dtype=torch.uint8, device=dev)
            st = torch.zeros((max_sf * 64,), dtype=torch.uint8, device=dev)
            res = torch.zeros((32,), dtype=torch.uint8, device=dev)
            pres = torch.zeros((64,), dtype=torch.uint8, device=dev)
            keep.append((data, st, res, pres))
            follow.append(dabgpu.DabplusEntry(outs[0][j].data_ptr(), 3 * br, br, carry[0][j].data_ptr() if call_no else None, carry[1][j].data_ptr(),
                                              data.data_ptr(), st.data_ptr(), res.data_ptr()))
            pads.append(dabgpu.PadEntry(data.data_ptr(), 110 * br // 8, st.data_ptr(), res.data_ptr(), br, max_sf,
                                        state[0][j].data_ptr() if call_no else None, state[1][j].data_ptr(), labels[j].data_ptr(), pres.data_ptr()))
            mots.append(dabgpu.MotEntry(data.data_ptr(), 110 * br // 8, st.data_ptr(), res.data_ptr(), br, max_sf,
                                        mstate[0][j].data_ptr() if call_no else None, mstate[1][j].data_ptr(), arenas[j].data_ptr(), arenas[j].numel(),
                                        slots[call_no, j].data_ptr(), 1024, 2, 0, results[call_no, j].data_ptr()))
        c.dabplus_follow_dev(follow, n_cifs)
        c.mot_slides_dev(mots)                                       # behind it on the same stream: nothing waits in between
        c.pad_labels_dev(pads)
        c.sync()
        for lst in (hist, carry, state, mstate):
            lst.reverse()
    got = labels.cpu().numpy().view(dabgpu.PAD_LABEL_DTYPE).reshape(2)
    counts = results.cpu().numpy().view(dabgpu.MOT_RESULT_DTYPE).reshape(n_calls, 2)
    raw = slots.cpu().numpy()
    for j in range(2):
        assert dabgpu.pad_label_utf8(got[j]) == E2E_LABELS[j].decode("utf-8"), j
        assert counts[:, j]["slides_written"].tolist() == [1, 0, 0] and counts[:, j]["groups_crc_failed"].sum() == 0, counts[:, j]
        assert counts[:, j]["groups_repeated"].sum() >= 2 * len(E2E_OBJECTS[j][2])
        rec = raw[0, j, 0, :32].copy().view(dabgpu.MOT_SLIDE_DTYPE)
        header, body = E2E_OBJECTS[j][0], E2E_OBJECTS[j][1]
        assert (int(rec["transport_id"][0]), int(rec["content_type"][0]), int(rec["header_bytes"][0]), int(rec["body_bytes"][0])) == (0x1000 + j, 2, len(header), len(body))
        assert raw[0, j, 0, 32:32 + len(header)].tobytes() == header and raw[0, j, 0, 32 + len(header):32 + len(header) + len(body)].tobytes() == body
        assert dabgpu.mot_header_parse(header)["name"] == E2E_NAMES[j] and (raw[0, j, 1] == FILL).all() and (raw[1:, j] == FILL).all()


@pytest.mark.gpu
def test_demo_shows_both_slides_and_both_labels(built, tmp_path):
    """the host mirror on that IQ: Basic_DAB_Plus_Channel::Process runs the MOT walk beside the label walk, and
    dab_host_demo lists the slides of every channel's Basic_Slideshow_Manager"""
    host = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")
    if not os.path.exists(os.path.join(host, "dab_host_demo")):
        subprocess.check_call(["make", "-C", host, "-j4"], stdout=subprocess.DEVNULL)
    ens = synth.ServiceEnsemble(E2E_SEED, E2E_SERVICES, n_frames=5, extras=False, bodies=e2e_bodies()[0])
    iq = np.tile(ens.iq().ravel(), 3)
    iq = synth.channel(iq, snr_db=20.0, cfo=0.4 / 2048, rng=np.random.default_rng(21))
    path = tmp_path / "iq.cf32"
    np.concatenate([iq[-30000:], iq, iq[:synth.NB_NULL + 5000]]).astype(np.complex64).tofile(path)
    prefix = str(tmp_path / "out")
    r = subprocess.run([os.path.join(host, "dab_host_demo"), str(path), prefix, "40000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "frames_desync=0" in r.stdout, r.stdout + r.stderr
    check_demo_database(prefix + ".db")


def check_demo_database(path):
    """the .db file of dab_host_demo: both channels with their labels, one slide each, name and image as sent"""
    lines = open(path).read().splitlines()
    chans = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith("channel")]
    slides = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith("slide ")]
    assert [int(ch["subchannel"]) for ch in chans] == [3, 7] and [int(sl["subchannel"]) for sl in slides] == [3, 7]
    for j, (ch, sl) in enumerate(zip(chans, slides)):
        assert bytes.fromhex(ch["label"]) == E2E_LABELS[j] and ch["label_charset"] == "15", ch
        assert int(sl["tid"]) == 0x1000 + j and bytes.fromhex(sl["name"]) == E2E_NAMES[j], sl
        assert int(sl["bytes"]) == len(E2E_OBJECTS[j][1]) and bytes.fromhex(sl["body"]) == E2E_OBJECTS[j][1]


def test_mirror_runs_the_shared_walks_and_needs_no_new_abi_symbol():
    host = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")
    src = open(os.path.join(host, "basic_radio", "basic_dab_plus_channel.cpp")).read()
    hdr = open(os.path.join(host, "basic_radio", "basic_dab_plus_channel.h")).read()
    assert '#include "dabgpu_mot_walk.h"' in hdr and "dabgpu_mot::walk_au(" in src and "dabgpu_mot::parse_header(" in src
    assert "dabgpu_mot_slides" not in src + hdr and "dabgpu_mot_header_parse" not in src + hdr
    assert "dabgpu_mot" not in open(os.path.join(ROOT, "tests", "fake_abi", "fake_dabgpu.cpp")).read()
    walk = open(os.path.join(ROOT, "include", "dabgpu_pad_walk.h")).read()
    mot = open(os.path.join(ROOT, "include", "dabgpu_mot_walk.h")).read()
    assert walk.count("walk_fields(") == 2 and "pad::walk_fields(k, au, len)" in mot           # one field walk, two sinks


def test_mirror_over_the_fake_abi_shows_both_slides_and_both_labels(built, tmp_path):
    """the same, without a GPU: dab_host_demo and the mirror over the TEST-ONLY fake ABI of tests/fake_abi (the oracle behind
    the mirror; never shipped), on the end-to-end IQ"""
    host, fake, oracle = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host"), os.path.join(ROOT, "tests", "fake_abi"), os.path.join(ROOT, "oracle")
    exe = str(tmp_path / "dab_host_demo_fake")
    srcs = [os.path.join(host, "demo", "dab_host_demo.cpp"), os.path.join(fake, "fake_dabgpu.cpp")]
    srcs += [os.path.join(host, s) for s in ("ofdm/ofdm_demodulator.cpp", "basic_radio/basic_radio.cpp", "basic_radio/basic_dab_plus_channel.cpp", "dab/fic/fic_parser.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I" + host, "-I" + os.path.join(ROOT, "include"), "-I" + oracle, "-I" + fake] + srcs +
                          ["-L" + oracle, "-loracle", "-Wl,-rpath," + oracle, "-o", exe])
    ens = synth.ServiceEnsemble(E2E_SEED, E2E_SERVICES, n_frames=5, extras=False, bodies=e2e_bodies()[0])
    iq = np.tile(ens.iq().ravel(), 3)
    iq = synth.channel(iq, snr_db=20.0, cfo=0.4 / 2048, rng=np.random.default_rng(21))
    path = tmp_path / "iq.cf32"
    np.concatenate([iq[-30000:], iq, iq[:synth.NB_NULL + 5000]]).astype(np.complex64).tofile(path)
    prefix = str(tmp_path / "out")
    r = subprocess.run([exe, str(path), prefix, "40000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "frames_desync=0" in r.stdout, r.stdout + r.stderr
    check_demo_database(prefix + ".db")
