"""dabgpu_packet_slides_dev / dabgpu_packet_slides_host (the slideshow objects of packet-mode MOT service components, from the
logical frames of their sub-channel) and dabgpu_fig_packet_components, against tests/packet_reference.py: slides, counters
byte for byte and count for count -- no tolerance anywhere -- every output between sentinel bytes.

The cases are streams of logical frames (STREAMS), each about one clause of the contract: the CPU tests take each through
dabgpu_packet_slides_host, whole and cut into calls with state and arena handed on, and check on the reference's own figures
that the stream is what its name says; the GPU tests take all of them in one call, and the shapes only a device can get
wrong.  The transmit side is dabgpu/synth.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import mot_reference as M
import packet_reference as R
from conftest import ROOT
from test_device_asm import CSRC, kernel_metadata

ARG, CAPACITY = -1, -6
FILL, GAP = 0xA7, 64
ADDR = 7


# ------------------------------------------------------------------------------------------------ building streams
def image(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def obj(tid, nbytes, seed, name, seg, hseg=None):
    """-> (header bytes, body bytes, data groups: header's, then body's)"""
    body = image(nbytes, seed)
    header = synth.slide_header(len(body), name)
    return header, body, synth.mot_object_groups(tid, header, body, seg, hseg)


def renumber(packets, ci=0):
    """the packets with continuity indices ci, ci + 1, ... (and the CRC that goes with them)"""
    out = []
    for k, p in enumerate(packets):
        body = bytes([(p[0] & 0xCF) | (((ci + k) & 3) << 4)]) + bytes(p[1:-2])
        c = synth.crc16(body)
        out.append(body + bytes([c >> 8, c & 0xFF]))
    return out


PAD1 = synth.padding_packet(1)


def frame(S, *items, cut=False):
    """one logical frame of S slots: the items back to back (cut: what overruns the frame is cut off), then padding packets"""
    blob = b"".join(bytes(i) for i in items)
    if cut:
        blob = blob[:24 * S]
    assert len(blob) <= 24 * S and len(blob) % 24 == 0, (len(blob), S)
    blob += PAD1 * (S - len(blob) // 24)
    return np.frombuffer(blob, np.uint8)


def frames_of(S, rows):
    return np.stack([frame(S, *r) for r in rows])


def exact_packets(groups, address, sizes):
    """data groups in packets of exactly sizes[k % len] slots (k: the running packet number), whatever is left of the group"""
    out, k = [], 0
    for g in groups:
        at = 0
        while True:
            L = sizes[k % len(sizes)]
            take = min(len(g) - at, 24 * L - 5)
            out.append(synth.packet(address, g[at:at + take], L, ci=k, first=at == 0, last=at + take == len(g)))
            k, at = k + 1, at + take
            if at == len(g):
                break
    return out


def one(data, first=True, last=True, slots=None, **kw):
    return synth.packet(ADDR, data, slots, first=first, last=last, **kw)


def sent(*objs):
    return [(tid, o[0], o[1]) for tid, o in objs]


def _streams():
    S = {}
    # every packet length at every position of a frame of six slots, and every one that overruns it
    o = obj(0x100, 1500, 1, b"lengths.jpg", 400)
    pk = exact_packets(o[2], ADDR, (1, 2, 3, 4))
    rows, at, places = [], {1: 0, 2: 0, 3: 0, 4: 0}, set()
    for p in pk:
        L = len(p) // 24
        pos = at[L] % (6 - L + 1)
        at[L] += 1
        places.add((L, pos))
        rows.append([PAD1] * pos + [p])
    assert places == {(L, pos) for L in range(1, 5) for pos in range(0, 7 - L)}, sorted(places)
    over = [(L, pos) for L in range(2, 5) for pos in range(7 - L, 6)]
    for j, (L, pos) in enumerate(over):                               # (never good: no continuity index is spent on them)
        rows.insert(3 + 4 * j, (L, pos))
    frames = np.stack([frame(6, *([PAD1] * r[1] + [one(b"", slots=r[0])]), cut=True) if isinstance(r, tuple) else frame(6, *r) for r in rows])
    S["lengths"] = dict(bitrate=48, frames=frames, slides=sent((0x100, o)), body_capacity=2048, slide_stride=2048,
                        counts=dict(slots_bad=sum(6 - pos for _L, pos in over), packets_followed=len(pk), continuity_breaks=0, slides_written=1))
    # resynchronisation: a bad slot in front of good packets; a bad packet of 96 bytes with a good one inside it
    o = obj(0x110, 300, 2, b"resync.jpg", 120)
    pk = synth.packetise(o[2], ADDR, sizes=(2,))
    assert len(pk) >= 5 and len(pk[2]) == 48
    bad1 = one(b"never", crc=False)
    bad4 = bytes([0xC0 | (ADDR >> 8), ADDR & 0xFF, 0x11]) + bytes(21) + pk[2] + bytes(24)
    assert len(bad4) == 96 and bad4[0] >> 6 == 3
    rows = [[bad1, pk[0], pk[1]], [bad4]] + [[p] for p in pk[3:]]
    S["resync"] = dict(bitrate=64, frames=frames_of(8, rows), slides=sent((0x110, o)), body_capacity=512,
                       counts=dict(slots_bad=3, packets_followed=len(pk), continuity_breaks=0, slides_written=1))
    # an all-zero frame and random frames: NOISE_SEED is the first seed whose three random frames of 64 slots hold a good CRC
    # by accident (test_noise_seed_gives_an_accidental_good_crc holds it to that)
    noise = np.random.default_rng(NOISE_SEED).integers(0, 256, (3, 1536), dtype=np.uint8)
    S["noise"] = dict(bitrate=512, frames=np.concatenate([np.zeros((1, 1536), np.uint8), noise]), slides=[], body_capacity=64, counts=dict(cifs=4, slots=256))
    # padding, other addresses, address 1022: an FEC-shaped slot, a good packet of one slot and one of two
    o = obj(0x120, 100, 3, b"addresses.jpg", 64)
    pk = synth.packetise(o[2], ADDR, sizes=(1,))
    rng = np.random.default_rng(5)
    others = [synth.packet(5, b"other", 1), synth.packet(1023, b"other", 2), synth.packet(1022, b"good", 1), synth.packet(1022, b"good", 2)]
    rows = [[pk[0], others[0], synth.fec_packet(rng), others[2]], [synth.padding_packet(3), others[3], pk[1]]] + [[synth.fec_packet(rng), p, others[1]] for p in pk[2:]]
    n_fec = 1 + len(pk) - 2
    for fec in (0, 1):
        S["addresses, fec %d" % fec] = dict(
            bitrate=64, frames=frames_of(8, rows), fec=fec, slides=sent((0x120, o)), body_capacity=256,
            counts=dict(packets_fec=(n_fec + 1) * fec, slots_bad=n_fec * (1 - fec), packets_other=2 + len(pk) - 2 + (1 - fec), packets_followed=len(pk)))
    # every continuity value, a break at each, and one in mid-group
    g = synth.msc_data_group(6, b"continuity")
    cis = [0, 1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2, 0, 1, 2, 3, 1]
    rows = [[one(g, ci=ci)] for ci in cis] + [[one(g[:5], last=False, ci=2)], [one(g[5:], first=False, ci=0)], [one(g, ci=1)]]
    S["continuity"] = dict(bitrate=32, frames=frames_of(4, rows), slides=[], body_capacity=64,
                           counts=dict(continuity_breaks=5, groups_unfinished=1, packets_orphan=1, groups_ignored_type=len(cis) + 1))
    # useful data lengths: 0, the most a packet of each size holds, one more than that
    g = synth.msc_data_group(6, bytes(19 + 43 + 67 + 91 - 4))
    cuts = [0, 0, 19, 62, 129, 220]
    pk = [one(g[cuts[i]:cuts[i + 1]], first=i == 0, last=i == 4, slots=max(i, 1)) for i in range(5)]
    again = synth.msc_data_group(6, b"again")
    pk += [one(b"open", last=False), one(bytes(19), slots=1, udl=20), one(again), one(bytes(91), slots=4, udl=92), one(bytes(10), slots=1, udl=127)]
    S["useful lengths"] = dict(bitrate=64, frames=frames_of(8, [[p] for p in renumber(pk)]), slides=[], body_capacity=64,
                               counts=dict(packets_malformed=3, groups_unfinished=1, groups_ignored_type=2, group_bytes=220 + 4 + len(again), groups_opened=3))
    # command packets inside a group
    o = obj(0x130, 200, 4, b"commands.jpg", 90)
    pk = synth.packetise(o[2], ADDR, sizes=(2,))
    cmd = synth.packet(ADDR, b"\x01\x02", 1, first=True, last=True, command=True)
    pk = [pk[0], cmd] + pk[1:3] + [cmd, cmd] + pk[3:]
    S["commands"] = dict(bitrate=64, frames=frames_of(8, [renumber(pk)[i:i + 2] for i in range(0, len(pk), 2)]), slides=sent((0x130, o)), body_capacity=256,
                         counts=dict(packets_command=3, continuity_breaks=0, groups_unfinished=0))
    # orphans, a first packet while a group is open, a group of one packet; groups of 3 and 4 bytes
    o = obj(0x140, 40, 5, b"one.jpg", 64)
    assert all(len(x) <= 91 for x in o[2])
    pk = [one(b"orphan", first=False, last=False), one(b"orphan", first=False), one(o[2][0][:9], last=False), one(o[2][0]), one(o[2][1]),
          one(b"\x46\x00\x00"), one(synth.msc_data_group(6, b"")), one(b"\x46\x00\x12\x34"), one(b"")]
    assert len(synth.msc_data_group(6, b"")) == 4
    S["small"] = dict(bitrate=64, frames=frames_of(8, [renumber(pk)[i:i + 3] for i in range(0, len(pk), 3)]), slides=sent((0x140, o)), body_capacity=64,
                      counts=dict(packets_orphan=2, groups_unfinished=1, groups_opened=7, groups_malformed=2, groups_ignored_type=1, groups_crc_failed=1, groups_ok=2))
    # groups of 16384 and 16385 bytes
    g0, g1 = synth.msc_data_group(6, bytes(16384 - 4)), synth.msc_data_group(6, bytes(16385 - 4))
    pk = synth.packetise([g0, g1, synth.msc_data_group(6, b"after")], ADDR, sizes=(4,))
    S["long"] = dict(bitrate=512, frames=synth.packet_frames(512, [pk]), slides=[], body_capacity=64,
                     counts=dict(groups_too_long=1, groups_ignored_type=2, groups_crc_failed=0, packets_orphan=0, group_bytes=16384 + 16380 + len(synth.msc_data_group(6, b"after"))))
    # repeated objects and more objects than slots; a slot too small
    small = [obj(0x150 + i, 60 + i, 10 + i, b"s%d" % i, 64) for i in range(3)]
    pk = synth.packetise(small[0][2] + small[0][2] + small[1][2] + small[2][2], ADDR, sizes=(2, 1))
    S["slots"] = dict(bitrate=64, frames=synth.packet_frames(64, [pk]), slides=sent((0x150, small[0]), (0x151, small[1])), body_capacity=256, max_slides=2,
                      counts=dict(groups_repeated=len(small[0][2]), objects_completed=3, slides_written=2, slides_dropped=1))
    S["slot too small"] = dict(bitrate=64, frames=synth.packet_frames(64, [synth.packetise(small[0][2], ADDR)]), slides=[], body_capacity=256, slide_stride=48,
                               counts=dict(objects_completed=1, slides_dropped=1))
    # one sub-channel, three addresses
    three = [obj(0x160 + i, 500 + 30 * i, 20 + i, b"shared %d" % i, 150) for i in range(3)]
    shared = synth.packet_frames(128, [synth.packetise(three[i][2], a, sizes=(4, 2, 3)) for i, a in enumerate((ADDR, 8, 300))])
    for i, a in enumerate((ADDR, 8, 300)):
        S["shared, address %d" % a] = dict(bitrate=128, frames=shared, address=a, slides=sent((0x160 + i, three[i])), body_capacity=1024, share="shared, address 7",
                                           counts=dict(slides_written=1, continuity_breaks=0))
    # the bit rates: S = 1, 3, 9 (frames that do not divide a wave), 32 and 64; 68 frames each, more than a wave's worth at S < 64
    for i, (br, nbytes) in enumerate(((8, 500), (24, 1200), (72, 2500), (256, 9000), (512, 20000))):
        a, b = obj(0x200 + 2 * i, nbytes, 30 + i, b"rate %d a" % br, 1000), obj(0x201 + 2 * i, nbytes // 2, 40 + i, b"rate %d b" % br, 333)
        pk = synth.packetise(a[2] + b[2], ADDR, sizes=(4, 1, 3, 2) if br > 24 else (br // 8,))
        beside = synth.packetise(obj(0x300 + i, nbytes // 3, 50 + i, b"beside", 200)[2], 9, sizes=(min(4, br // 8),))
        fr = synth.packet_frames(br, [pk, beside] if br > 8 else [pk], n_frames=68)
        assert len(fr) == 68, (br, len(fr))
        S["rate %d" % br] = dict(bitrate=br, frames=fr, slides=sent((0x200 + 2 * i, a), (0x201 + 2 * i, b)), body_capacity=20000, slide_stride=20480 + 256,
                                 counts=dict(slides_written=2, continuity_breaks=0, slots_bad=0))
    return S


NOISE_SEED = 113
STREAMS = None


def streams():
    global STREAMS
    if STREAMS is None:
        STREAMS = _streams()
    return STREAMS


STREAM_NAMES = ["lengths", "resync", "noise", "addresses, fec 0", "addresses, fec 1", "continuity", "useful lengths", "commands", "small", "long",
                "slots", "slot too small", "shared, address 7", "shared, address 8", "shared, address 300", "rate 8", "rate 24", "rate 72", "rate 256",
                "rate 512"]


# ------------------------------------------------------------------------------------------------ one call, on any memory
class HostMemory:
    def load(self, img):
        raw = np.empty(img.size + 256, np.uint8)
        off = -raw.ctypes.data % 256
        self.buf = raw[off:off + img.size]
        self.buf[:] = img
        return self.buf.ctypes.data

    def run(self, entries, n_cifs):
        dabgpu.packet_slides_host(entries, n_cifs)

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
        self.ctx.packet_slides_dev(entries, n_cifs)
        self.ctx.sync()

    def read(self):
        self.ctx.sync()
        return self.t.cpu().numpy()


def stride_of(sp):
    return sp.get("slide_stride") or 1024


def spec_of(st, a=0, b=None, **kw):
    sp = {k: v for k, v in st.items() if k not in ("slides", "counts", "share")}
    sp["frames"] = st["frames"][a:b]
    sp.update(kw)
    return sp


def call(mem, specs, n_cifs, mutate=None, refused=None, shared=()):
    """One call on buffers laid out in one allocation, every region between sentinel bytes.  specs: dicts {bitrate, frames (at
    least n_cifs rows), address, fec, state (bytes or None = NULL), arena (bytes or None = sentinel bytes), body_capacity,
    max_slides, slide_stride, stride (in_stride), in_off (the frames begin that many bytes off their 256-byte boundary)};
    shared: {entry: the entry whose frames it names}.  After the call nothing but state-out, arena, result and the slots'
    written bytes may have changed (nothing at all for a refused call).  -> per entry dict(slides [(record, header, body)],
    result, state, arena)"""
    size, lay = 0, []

    def take(n):
        nonlocal size
        off = (size + GAP + 255) // 256 * 256
        size = off + n
        return off

    nb = dabgpu.packet_state_bytes()
    for e, sp in enumerate(specs):
        stride = sp.get("stride", 3 * sp["bitrate"])
        ab = dabgpu.mot_arena_bytes(sp["body_capacity"])
        frames = lay[shared[e]]["frames"] if e in shared else take(max(n_cifs, 1) * stride + 16) + sp.get("in_off", 0)
        lay.append(dict(frames=frames, sin=take(nb) if sp.get("state") is not None else None, sout=take(nb), arena=take(ab), ab=ab,
                        slides=take(max(sp.get("max_slides", 4), 1) * stride_of(sp)), result=take(192)))
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
    entries = [dabgpu.PacketEntry(base + L["frames"], sp.get("stride", 3 * sp["bitrate"]), sp["bitrate"], sp.get("address", ADDR), sp.get("fec", 0), 0,
                                  base + L["sin"] if L["sin"] is not None else None, base + L["sout"], base + L["arena"], L["ab"],
                                  base + L["slides"], stride_of(sp), sp.get("max_slides", 4), 0, base + L["result"]) for sp, L in zip(specs, lay)]
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
        for key, n in (("sout", nb), ("arena", L["ab"]), ("result", 192)):
            untouched[L[key]:L[key] + n] = False
        res = after[L["result"]:L["result"] + 192].copy().view(dabgpu.PACKET_RESULT_DTYPE)
        written = int(res["mot"]["slides_written"][0])
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


def receiver(sp):
    return R.Receiver(sp["body_capacity"], sp.get("address", ADDR), sp.get("fec", 0))


def ref_call(rx, sp, n_cifs=None):
    frames = sp["frames"] if n_cifs is None else sp["frames"][:n_cifs]
    return rx.call(frames, sp["bitrate"], sp.get("max_slides", 4), stride_of(sp))


_WANTS = {}


def wanted(name):
    """the reference's answer to a whole stream: computed once, shared, left as it is"""
    if name not in _WANTS:
        sp = spec_of(streams()[name])
        _WANTS[name] = ref_call(receiver(sp), sp)
    return _WANTS[name]


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_records_and_sizes(built, tmp_path):
    L = dabgpu.lib()
    for name in ("dabgpu_packet_state_bytes", "dabgpu_packet_slides_dev", "dabgpu_packet_slides_host", "dabgpu_fig_packet_components"):
        assert name in dabgpu.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.dabgpu_abi_version() == 6 == dabgpu.ABI_VERSION
    assert dabgpu.PACKET_RESULT_DTYPE.itemsize == 192 == R.RESULT_DTYPE.itemsize and dabgpu.PACKET_RESULT_DTYPE.names == R.RESULT_DTYPE.names
    assert dabgpu.PACKET_RESULT_DTYPE.fields["mot"][0] == dabgpu.MOT_RESULT_DTYPE
    assert dabgpu.packet_state_bytes() % 16 == 0 and dabgpu.packet_state_bytes() > dabgpu.mot_state_bytes() and hasattr(dabgpu.Context, "packet_slides_dev")
    # the binding's structures and the records against the header, as the C compiler lays them out
    structs = [("dabgpu_packet_entry", dabgpu.PacketEntry), ("dabgpu_packet_component", dabgpu.PacketComponent)]
    records = [("dabgpu_packet_result", dabgpu.PACKET_RESULT_DTYPE), ("dabgpu_packet_component", dabgpu.PACKET_COMPONENT_DTYPE)]
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
    p = synth.packet(0x2A5, b"abc", 2, ci=3, first=True, last=False)
    assert len(p) == 48 and p[0] == (1 << 6) | (3 << 4) | (1 << 3) | 0x02 and p[1] == 0xA5 and p[2] == 3 and p[3:6] == b"abc" and p[6:46] == bytes(40)
    assert R.crc(p[:46]) == int.from_bytes(p[46:], "big") and R.crc(synth.packet(1, b"x", crc=False)[:22]) != int.from_bytes(synth.packet(1, b"x", crc=False)[22:], "big")
    assert len(synth.packet(1, bytes(19))) == 24 and len(synth.packet(1, bytes(20))) == 48 and len(synth.packet(1, bytes(91))) == 96
    assert synth.packet(1, b"", command=True)[2] == 0x80 and synth.padding_packet(3)[:3] == bytes([0x8C, 0, 0])
    f = synth.fec_packet(np.random.default_rng(0))
    assert len(f) == 24 and f[0] >> 6 == 0 and ((f[0] & 3) << 8 | f[1]) == 1022
    pk = synth.packetise([bytes(100), b""], 9, sizes=(1, 2), ci=2)
    assert [len(x) // 24 for x in pk] == [1, 2, 1, 1, 1] and [(x[0] >> 4) & 3 for x in pk] == [2, 3, 0, 1, 2]
    assert [(x[0] >> 2) & 3 for x in pk] == [2, 0, 0, 1, 3] and [x[2] for x in pk] == [19, 43, 19, 19, 0]
    big = synth.packet(5, b"z", 4)
    fr = synth.packet_frames(32, [pk, [big]], n_frames=3)
    assert fr.shape == (3, 96) and fr[0].tobytes() == pk[0] + pk[1] + pk[2] and fr[1].tobytes() == pk[3] + pk[4] + synth.padding_packet(2)
    assert fr[2].tobytes() == big


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_host_equals_the_reference(built, name):
    """each stream in one call: slides and counters equal the reference's; the reference itself reports what the stream is
    about, and the objects that were sent"""
    st = streams()[name]
    sp = spec_of(st)
    want = wanted(name)
    got = call(HostMemory(), [sp], len(sp["frames"]))[0]
    assert same(got, want), name + explain(got, want)
    assert [(int(r["transport_id"][0]), h, b) for r, h, b in want[0]] == st["slides"], name
    for key, value in st["counts"].items():
        have = want[1][key] if key in R.COUNTERS else want[1]["mot"][key]
        assert int(have[0]) == value, (name, key, want[1])
    for key in ("aus", "aus_lost", "aus_with_xpad", "pad_malformed", "fields_ignored", "lengths_ok", "lengths_ignored", "groups_no_length", "xpad_bytes"):
        assert int(got["result"]["mot"][key][0]) == 0
    assert set(STREAM_NAMES) == set(streams())


def test_noise_seed_gives_an_accidental_good_crc(built):
    """the random frames of the noise stream hold at least one good packet CRC by accident (the scan takes it for a packet and
    steps over its slots), no smaller seed does, and the all-zero frame holds none"""
    def bad_slots(seed):
        fr = np.random.default_rng(seed).integers(0, 256, (3, 1536), dtype=np.uint8)
        return int(call(HostMemory(), [dict(bitrate=512, frames=fr, body_capacity=64)], 3)[0]["result"]["slots_bad"][0])
    assert all(bad_slots(seed) == 192 for seed in range(NOISE_SEED)) and bad_slots(NOISE_SEED) < 192
    res = wanted("noise")[1]
    good = int(res["packets_padding"][0] + res["packets_other"][0] + res["packets_followed"][0])
    assert good >= 1 and int(res["slots_bad"][0]) + good <= 256 - 1 + good and int(res["slots_bad"][0]) >= 64
    zero = call(HostMemory(), [dict(bitrate=512, frames=np.zeros((1, 1536), np.uint8), body_capacity=64)], 1)[0]["result"]
    assert int(zero["slots_bad"][0]) == 64


def run_cut(mem_of, st, cuts, **kw):
    """the stream in calls that end at `cuts` (and its end), state and arena handed on -> (slides of all calls, summed
    counters, last state)"""
    state, arena, at, slides, results = None, None, 0, [], []
    n = len(st["frames"])
    for end in list(cuts) + [n]:
        sp = spec_of(st, at, end, state=state, arena=arena, **kw)
        r = call(mem_of(), [sp], end - at)[0]
        state, arena, at = r["state"], r["arena"], end
        slides += r["slides"]
        results.append(r["result"])
    return slides, R.total(results), state


def strip(slides):
    """slides without where in their call they completed"""
    return [(int(r["transport_id"][0]), int(r["content_type"][0]), int(r["content_subtype"][0]), h, b) for r, h, b in slides]


@pytest.mark.parametrize("name", [n for n in STREAM_NAMES if n not in ("rate 256", "rate 512", "slots", "slot too small")])
def test_cut_into_two_and_three_calls_at_every_frame_boundary(built, name):
    """each stream cut into two calls at EVERY frame boundary and into three at every pair of neighbouring ones, state and
    arena carried: groups and objects span the calls; slides, summed counters and the last state record equal the uncut run's"""
    st = streams()[name]
    n = len(st["frames"])
    whole = run_cut(HostMemory, st, [], max_slides=4)
    want = wanted(name)
    assert strip(whole[0]) == strip(want[0]) and whole[1] == R.total([want[1]])
    for cuts in [[k] for k in range(0, n + 1)] + [[k, k + 1] for k in range(1, n - 1)]:
        got = run_cut(HostMemory, st, cuts, max_slides=4)
        assert strip(got[0]) == strip(whole[0]) and got[1] == whole[1], (name, cuts)
        assert got[2].tobytes() == whole[2].tobytes(), (name, cuts)


def test_a_foreign_state_record_is_a_fresh_start(built):
    st = streams()["commands"]
    rng = np.random.default_rng(7)
    sp = spec_of(st)
    n = len(sp["frames"])
    want = wanted("commands")
    for k in range(40):
        state = rng.integers(0, 256, dabgpu.packet_state_bytes(), dtype=np.uint8)
        if k % 2:                                                     # nearly ours: a record of this library's with one byte changed
            state = call(HostMemory(), [spec_of(st, 0, 2)], 2)[0]["state"]
            state[rng.integers(0, state.size)] ^= 1 << rng.integers(0, 8)
        got = call(HostMemory(), [dict(sp, state=state)], n)[0]       # (whatever it holds: nothing outside the outputs is written)
        if k % 2 == 0:
            assert same(got, want), k
    other = call(HostMemory(), [dict(spec_of(st, 0, 2), body_capacity=64)], 2)[0]["state"]
    assert same(call(HostMemory(), [dict(sp, state=other)], n)[0], want)


def spoil(field, value, at=-1):
    def f(entries):
        setattr(entries[at], field, value(entries[at]) if callable(value) else value)
    return f


#: each refused with DABGPU_ERR_ARG, the bad entry LAST in the table: nothing of the good ones before it is written
BAD_ENTRIES = [spoil("bitrate_kbps", 12), spoil("bitrate_kbps", 0), spoil("bitrate_kbps", 520), spoil("bitrate_kbps", -8), spoil("in_stride", 191),
               spoil("address", 0), spoil("address", 1024), spoil("address", -1), spoil("d_in", None),
               spoil("d_state_out", None), spoil("d_arena", None), spoil("d_slides", None), spoil("d_result", None),
               spoil("d_state_in", lambda e: e.d_state_in + 8), spoil("d_state_out", lambda e: e.d_state_out + 4),
               spoil("d_state_out", lambda e: e.d_state_in), spoil("d_state_out", lambda e: e.d_state_in + 16),
               spoil("d_state_out", lambda e: e.d_state_in - 16), spoil("d_arena", lambda e: e.d_arena + 8),
               spoil("d_slides", lambda e: e.d_slides + 4), spoil("d_result", lambda e: e.d_result + 1),
               spoil("arena_bytes", lambda e: dabgpu.mot_arena_bytes(0) - 16), spoil("arena_bytes", 0), spoil("max_slides", -1),
               spoil("slide_stride", 16), spoil("slide_stride", 1000), spoil("slide_stride", 1 << 31), spoil("max_slides", 1 << 21)]


def refusal_specs():
    st = streams()["commands"]
    zero = np.zeros(dabgpu.packet_state_bytes(), np.uint8)
    return [spec_of(st, state=zero) for _ in range(3)], len(st["frames"])


def test_refusals_that_need_no_device(built):
    L = dabgpu.lib()
    specs, n = refusal_specs()
    for m in BAD_ENTRIES:
        call(HostMemory(), specs, n, mutate=m, refused=ARG)
    good = (dabgpu.PacketEntry * 1)(dabgpu.PacketEntry(0x10000, 192, 64, 7, 0, 0, None, 0x40000, 0x50000, dabgpu.mot_arena_bytes(64), 0x60000, 1024, 1, 0, 0x70000))
    assert L.dabgpu_packet_slides_host(None, 1, 0) == ARG and L.dabgpu_packet_slides_host(good, -1, 0) == ARG
    assert L.dabgpu_packet_slides_host(good, 1, -1) == ARG and L.dabgpu_packet_slides_host(good, 1, (1 << 24) + 1) == ARG
    assert L.dabgpu_packet_slides_host(None, 0, 4) == 0
    assert L.dabgpu_packet_slides_dev(None, good, 1, 0, None) == ARG   # no context: refused before anything is looked for
    got = call(HostMemory(), specs, n)                                 # ... and the unspoilt table goes through
    assert all(same(r, wanted("commands")) for r in got)
    # d_slides may be NULL where there are no slots, d_in where there are no frames
    call(HostMemory(), [dict(specs[0], max_slides=0)], n, mutate=spoil("d_slides", None))
    none = call(HostMemory(), specs[:1], 0, mutate=spoil("d_in", None))[0]
    assert none["result"].tobytes() == bytes(192) and none["state"].tobytes() == call(HostMemory(), specs[:1], 0)[0]["state"].tobytes()


# ---- which components are packet mode
def fibs_of(figs):
    """-> fib [1][12][32], crc_ok [1][12]: the FIGs packed into FIBs, the rest empty FIBs"""
    packed = synth.pack_fibs(figs)
    fib = np.concatenate([packed, np.repeat(synth.pack_fibs([synth.fig0_0(0xC181, 0)]), 12 - len(packed), axis=0)]).reshape(1, 12, 32)
    return fib, np.ones((1, 12), np.uint8)


SUBCH = [{"id": 9, "start": 200, "option": 0, "level": 3, "size": 24}, {"id": 4, "start": 100, "option": 0, "level": 3, "size": 48},
         {"id": 30, "start": 300, "uep_index": 5}]


def components(figs, max_out=64):
    fib, ok = fibs_of(figs)
    return [(a.sid, a.scid, a.subchid, a.start_address, a.packet_address, a.dscty, a.dg_flag, a.fec_scheme, a.primary)
            for a in dabgpu.fig_packet_components(fib, ok, max_out)]


def test_fig_packet_components(built):
    sv16 = [{"sid": 0xE1C0, "components": [{"scid": 0x123, "primary": True}, {"scid": 0xABC, "primary": False}]},
            {"sid": 0xC221, "components": [{"subchannel": 30, "ascty": 63}]}]
    sv32 = [{"sid": 0xE0D01234, "components": [{"scid": 0x001}, {"scid": 0xFFF, "primary": False}, {"scid": 0x555}]}]
    f3 = [synth.fig0_3([{"scid": 0x123, "subchannel": 9, "address": 1023, "dscty": 60, "dg_flag": 0},
                        {"scid": 0xABC, "subchannel": 9, "address": 5, "dscty": 5, "dg_flag": 1, "caorg": 0xBEEF},
                        {"scid": 0x001, "subchannel": 4, "address": 1}]),
          synth.fig0_3([{"scid": 0xFFF, "subchannel": 4, "address": 1, "dscty": 24},               # the same (SubChId, address) again
                        {"scid": 0x555, "subchannel": 31, "address": 2}])]                           # a sub-channel FIG 0/1 does not announce
    figs = [synth.fig0_1(SUBCH), synth.fig0_2(sv16), synth.fig0_2(sv32, pd=1)] + f3 + [synth.fig0_14([(9, 1), (30, 2)])]
    want = [(0xE0D01234, 0x001, 4, 100, 1, 60, 0, 0, 1), (0xE1C0, 0xABC, 9, 200, 5, 5, 1, 1, 0), (0xE1C0, 0x123, 9, 200, 1023, 60, 0, 1, 1)]
    assert components(figs) == want
    # a missing FIG 0/3: its component is left out; FIBs whose CRC failed are not read
    assert components([synth.fig0_1(SUBCH), synth.fig0_2(sv16), synth.fig0_2(sv32, pd=1), f3[1]]) == [(0xE0D01234, 0xFFF, 4, 100, 1, 24, 0, 0, 0)]
    assert components([synth.fig0_1(SUBCH), synth.fig0_2(sv16), f3[0]]) == [(0xE1C0, 0xABC, 9, 200, 5, 5, 1, 0, 0), (0xE1C0, 0x123, 9, 200, 1023, 60, 0, 0, 1)]
    assert components([synth.fig0_2(sv16), f3[0]]) == []                                            # no sub-channel organisation
    fib, ok = fibs_of(figs)
    ok[:] = 0
    assert dabgpu.fig_packet_components(fib, ok) == []
    # another configuration (C/N = 1) and another ensemble (OE = 1) are not this one
    other = [synth.fig0(3, f3[0][2:], cn=1), synth.fig0(3, f3[0][2:], oe=1)]
    assert components([synth.fig0_1(SUBCH), synth.fig0_2(sv16)] + other) == []
    # capacity and arguments
    L = dabgpu.lib()
    fib, ok = fibs_of(figs)
    arr, n = (dabgpu.PacketComponent * 4)(), C.c_int(-1)
    C.memset(arr, 0x5A, C.sizeof(arr))
    assert L.dabgpu_fig_packet_components(fib.ctypes.data, ok.ctypes.data, 1, arr, 2, C.byref(n)) == CAPACITY and n.value == 3
    assert bytes(arr) == b"\x5a" * C.sizeof(arr)
    assert L.dabgpu_fig_packet_components(fib.ctypes.data, ok.ctypes.data, 1, None, 0, C.byref(n)) == CAPACITY and n.value == 3
    assert L.dabgpu_fig_packet_components(fib.ctypes.data, ok.ctypes.data, 1, arr, 3, C.byref(n)) == 0 and n.value == 3
    assert L.dabgpu_fig_packet_components(None, ok.ctypes.data, 1, arr, 4, C.byref(n)) == ARG
    assert L.dabgpu_fig_packet_components(fib.ctypes.data, ok.ctypes.data, 1, None, 4, C.byref(n)) == ARG
    assert L.dabgpu_fig_packet_components(fib.ctypes.data, ok.ctypes.data, 1, arr, 4, None) == ARG
    # the audio components of the same FIBs are what they were: packet components are none of them
    assert [(a.sid, a.subchid) for a in dabgpu.fig_audio_components(fib, ok)] == [(0xC221, 30)]


# ---- device code, sanitizers
def test_new_kernels_neither_spill_nor_use_scratch(built, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the device assembly cannot be checked")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "packet_kernels.hip" in mk and "dabgpu_packet_api.hip" in mk
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    out = tmp_path / "packet_kernels.s"
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "packet_kernels.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    md = kernel_metadata(out.read_text())
    assert len(md) == 2 and sum("packet_scan_kernel" in k for k in md) == 1 and sum("packet_walk_kernel" in k for k in md) == 1
    for k, v in md.items():
        print("%s: vgprs %s, sgprs %s, LDS %s bytes" % (k, v.get("vgpr_count"), v.get("sgpr_count"), v.get("group_segment_fixed_size")))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)


def test_walk_fuzz_under_sanitizers(tmp_path):
    """tests/packet_walk_fuzz.cpp: scans and walks over random frames and mutated-valid ones, each a heap block of exactly its
    size, the staged packet, the arena and the slots exactly sized too, the copy orders executed with their bounds asserted;
    a stand-alone program built with the host compiler under AddressSanitizer and UBSan and run as a child process"""
    exe = str(tmp_path / "packet_walk_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "packet_walk_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "60000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "frames=60000" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = dict(kv.split("=") for kv in r.stdout.split())
    print(r.stdout)
    for key in ("slides", "dropped", "too_long", "malformed", "breaks", "orphan", "command", "fec", "bad", "repeated", "crc_failed"):
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
    turns, different slot counts, the three entries of the shared sub-channel naming the same frames"""
    specs, shared, index = [], {}, {}
    for e, name in enumerate(STREAM_NAMES):
        st = streams()[name]
        sp = spec_of(st, 0, n_cifs, max_slides=st.get("max_slides", [4, 2, 5][e % 3]))
        index[name] = e
        if st.get("share") and st["share"] != name:
            shared[e] = index[st["share"]]
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
def test_gpu_every_case_in_one_call(pctx):
    """all streams in ONE call of 68 logical frames (rows of 0xFF behind the shorter streams): bit rates from 8 to 512, three
    entries on one d_in, in_stride beyond 3 R, d_in off 16 and off 4 bytes: slides, counters, state record and arena equal the
    reference and the host call"""
    specs, shared = all_specs()
    specs = padded(specs, 68)
    wants = [ref_call(receiver(sp), sp) for sp in specs]
    got = call(DeviceMemory(pctx), specs, 68, shared=shared)
    host = call(HostMemory(), specs, 68, shared=shared)
    for name, g, h, w in zip(STREAM_NAMES, got, host, wants):
        assert same(g, w), name + explain(g, w)
        assert same(h, w), name
        assert g["state"].tobytes() == h["state"].tobytes() and (g["arena"] == h["arena"]).all(), name
    assert sum(len(g["slides"]) for g in got) >= 18 and sum(int(g["result"]["mot"]["slides_dropped"][0]) for g in got) >= 2


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
    """130 entries: thirteen streams of at most 23 frames, ten times over, each with outputs of its own"""
    names = [n for n in STREAM_NAMES if len(streams()[n]["frames"]) <= 23][:13]
    assert len(names) == 13
    specs = padded([spec_of(streams()[n], stride=3 * streams()[n]["bitrate"] + 3 * (k % 2)) for k in range(10) for n in names], 23)
    got = call(DeviceMemory(pctx), specs, 23)
    wants = {n: ref_call(receiver(sp), sp) for n, sp in zip(names, specs)}
    for k, g in enumerate(got):
        assert same(g, wants[names[k % 13]]), (k, names[k % 13])


@pytest.mark.gpu
def test_gpu_two_calls_back_to_back_with_the_state_on_the_device(pctx):
    """every stream in two calls enqueued one behind the other, nothing waiting in between: the state record of the first is
    the second's input, the arena stays in place: slides and summed counters equal the uncut host run's, the last state too"""
    import torch
    cut = 5
    names = [n for n in STREAM_NAMES if not n.startswith("slot") and len(streams()[n]["frames"]) >= 2 * cut]
    assert len(names) >= 12
    nb = dabgpu.packet_state_bytes()
    bufs = {}
    for name in names:
        st = streams()[name]
        n, stride = len(st["frames"]), stride_of(st)
        bufs[name] = dict(frames=torch.from_numpy(st["frames"]).cuda(), states=torch.zeros((2, nb), dtype=torch.uint8, device="cuda"),
                          arena=torch.full((dabgpu.mot_arena_bytes(st["body_capacity"]),), FILL, dtype=torch.uint8, device="cuda"),
                          slides=torch.full((2, 4, stride), FILL, dtype=torch.uint8, device="cuda"), results=torch.zeros((2, 192), dtype=torch.uint8, device="cuda"),
                          stride=stride)
    for k in range(2):
        entries = []
        for name in names:
            b, st = bufs[name], streams()[name]
            entries.append(dabgpu.PacketEntry(b["frames"][cut * k].data_ptr(), 3 * st["bitrate"], st["bitrate"], st.get("address", ADDR), st.get("fec", 0), 0,
                                              b["states"][1].data_ptr() if k else None, b["states"][k ^ 1].data_ptr(), b["arena"].data_ptr(), b["arena"].numel(),
                                              b["slides"][k].data_ptr(), b["stride"], 4, 0, b["results"][k].data_ptr()))
        pctx.packet_slides_dev(entries, cut)
    pctx.sync()
    for name in names:
        b, st = bufs[name], streams()[name]
        short = dict(st, frames=st["frames"][:2 * cut])
        whole = run_cut(HostMemory, short, [], max_slides=4)
        res = b["results"].cpu().numpy().view(dabgpu.PACKET_RESULT_DTYPE).reshape(2)
        raw = b["slides"].cpu().numpy()
        slides = []
        for k in range(2):
            for j in range(int(res[k]["mot"]["slides_written"])):
                rec = raw[k, j, :32].copy().view(dabgpu.MOT_SLIDE_DTYPE)
                hb, bb = int(rec["header_bytes"][0]), int(rec["body_bytes"][0])
                slides.append((rec, raw[k, j, 32:32 + hb].tobytes(), raw[k, j, 32 + hb:32 + hb + bb].tobytes()))
                assert (raw[k, j, 32 + hb + bb:] == FILL).all()
            assert (raw[k, int(res[k]["mot"]["slides_written"]):] == FILL).all()
        assert strip(slides) == strip(whole[0]), name
        assert R.total([res[k:k + 1] for k in range(2)]) == whole[1], name
        assert b["states"][0].cpu().numpy().tobytes() == whole[2].tobytes(), name


@pytest.mark.gpu
def test_gpu_refused_calls_leave_every_output_alone(pctx):
    specs, n = refusal_specs()
    for m in BAD_ENTRIES:
        call(DeviceMemory(pctx), specs, n, mutate=m, refused=ARG)
    pctx.packet_slides_dev([], 4)                                     # nothing to do is not an error
    got = call(DeviceMemory(pctx), specs, n)
    assert all(same(r, wanted("commands")) for r in got)


# ---- end to end
E2E_SEED = 3
E2E_DABPLUS = [("Radio One", 0xC221, 3, 0, 3, 64, 0)]
E2E_NAME = b"logo-0xD301.png"
E2E_OBJECT = obj(0x500, 600, 77, E2E_NAME, 300)
E2E_SCID, E2E_SUBCH, E2E_START = 0x123, 9, 48


def e2e_ensemble():
    """one ensemble: a DAB+ service of 64 kbit/s, and a packet-mode sub-channel of 32 kbit/s that carries the slide twice in its
    cycle of 20 logical frames"""
    pk = synth.packetise(E2E_OBJECT[2] + E2E_OBJECT[2], ADDR, sizes=(4,))
    while len(pk) % 4:                                                # (command packets, so that the continuity index goes on where the cycle wraps)
        pk.append(synth.packet(ADDR, b"\x00", 1, ci=len(pk), command=True))
    frames = synth.packet_frames(32, [pk], n_frames=20)
    assert frames.shape == (20, 96)
    service = ("Slides", 0xD301, E2E_SUBCH, 0, 3, 32, E2E_START, [(E2E_SCID, ADDR, synth.DSCTY_MOT, 0)], frames, 0)
    return synth.ServiceEnsemble(E2E_SEED, E2E_DABPLUS, n_frames=5, extras=False, packet_services=[service]), frames


def test_end_to_end_multiplex_announces_and_carries_the_slide(built):
    """what the GPU test will receive: the component list of the transmitted FIBs, and the reference receiver on the
    transmitted logical frames, two cycles of them"""
    ens, frames = e2e_ensemble()
    comps = dabgpu.fig_packet_components(ens.fibs, np.ones((5, 12), np.uint8))
    assert [(c.sid, c.scid, c.subchid, c.start_address, c.packet_address, c.dscty, c.dg_flag, c.fec_scheme, c.primary) for c in comps] == \
        [(0xD301, E2E_SCID, E2E_SUBCH, E2E_START, ADDR, 60, 0, 0, 1)]
    assert [(a.sid, a.subchid, a.ascty) for a in dabgpu.fig_audio_components(ens.fibs, np.ones((5, 12), np.uint8))] == [(0xC221, 3, 63)]
    slides, counts = R.Receiver(1024, ADDR).call(np.concatenate([frames, frames]), 32, 2, 1024)
    assert strip(slides) == [(0x500, 2, 1, E2E_OBJECT[0], E2E_OBJECT[1])] and dabgpu.mot_header_parse(slides[0][1])["name"] == E2E_NAME
    assert int(counts["mot"]["groups_repeated"][0]) == 3 * len(E2E_OBJECT[2]) and int(counts["continuity_breaks"][0]) == 0


@pytest.mark.gpu
def test_gpu_end_to_end_iq_to_slides(pctx):
    """IQ of 16 transmission frames of that ensemble -> front end -> FIC pass -> fig_subchannels and fig_packet_components ->
    decode_ensembles_dev -> packet_slides_dev behind it on the same stream, nothing waiting in between: the slide as sent,
    once; its second copy counted as repeated"""
    import torch
    dev = torch.device("cuda", 0)
    fps, L, FB = 16, 76 * 2552, dabgpu.NB_FRAME_BITS
    ens, _frames = e2e_ensemble()
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
    state = torch.zeros(dabgpu.packet_state_bytes(), dtype=torch.uint8, device=dev)
    arena = torch.zeros(dabgpu.mot_arena_bytes(1024), dtype=torch.uint8, device=dev)
    slots = torch.full((2, 1024), FILL, dtype=torch.uint8, device=dev)
    result = torch.zeros(192, dtype=torch.uint8, device=dev)
    c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), [plan], None, [[h.data_ptr() for h in hist]],
                           [[o.data_ptr() for o in outs]], None)
    c.packet_slides_dev([dabgpu.PacketEntry(outs[j].data_ptr(), 3 * br, br, comps[0].packet_address, comps[0].fec_scheme, 0, None, state.data_ptr(),
                                            arena.data_ptr(), arena.numel(), slots.data_ptr(), 1024, 2, 0, result.data_ptr())], n_cifs)
    c.sync()                                                          # (the only wait behind the decode call)
    res = result.cpu().numpy().view(dabgpu.PACKET_RESULT_DTYPE)
    raw = slots.cpu().numpy()
    header, body = E2E_OBJECT[0], E2E_OBJECT[1]
    assert int(res["mot"]["slides_written"][0]) == 1 and int(res["mot"]["groups_crc_failed"][0]) == 0, res
    assert int(res["mot"]["groups_repeated"][0]) >= len(E2E_OBJECT[2]) and int(res["cifs"][0]) == n_cifs, res
    rec = raw[0, :32].copy().view(dabgpu.MOT_SLIDE_DTYPE)
    assert (int(rec["transport_id"][0]), int(rec["content_type"][0]), int(rec["header_bytes"][0]), int(rec["body_bytes"][0])) == (0x500, 2, len(header), len(body))
    assert raw[0, 32:32 + len(header)].tobytes() == header and raw[0, 32 + len(header):32 + len(header) + len(body)].tobytes() == body
    assert dabgpu.mot_header_parse(header)["name"] == E2E_NAME and (raw[0, 32 + len(header) + len(body):] == FILL).all() and (raw[1] == FILL).all()
