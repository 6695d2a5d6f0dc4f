"""dabgpu_packet_groups_dev / dabgpu_packet_groups_host (the MSC data groups, or the raw bytes, of any packet-mode service
component) and dabgpu_fig_user_applications, against tests/data_groups_reference.py: emitted bytes, records, counters and the
state record byte for byte and count for count -- no tolerance anywhere -- every output between sentinel bytes.

The cases are streams of logical frames (STREAMS), each about one clause of the contract.  For every stream the named counts
are asserted on the REFERENCE's result first, so a stream is shown to be what its name says before the code under test is
held to it.  The CPU tests take each stream through dabgpu_packet_groups_host, whole and cut into two calls at every frame
boundary with the state handed on; the GPU tests take all of them in one call, and the seams only the kernel has (W = the
packets it takes at a time).  The transmit side is dabgpu/synth.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import data_groups_reference as R
from conftest import ROOT
from test_device_asm import CSRC, kernel_metadata

ARG, CAPACITY = -1, -6
FILL, GAP = 0xA7, 64
ADDR = 7
GROUP_CAP = 16384
STATE_DTYPE = np.dtype([("seen", np.uint8), ("prev", np.uint8), ("open", np.uint8), ("pad", np.uint8), ("have", np.uint16),
                        ("crc", np.uint16), ("type_mask", np.uint16), ("reserved", np.uint8, (6,)), ("last_ci", np.uint8, (16,)),
                        ("group", np.uint8, (GROUP_CAP,))])


# ------------------------------------------------------------------------------------------------ building streams
def payload(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def with_crc(g):
    c = synth.crc16(g)
    return bytes(g) + bytes([c >> 8, c & 0xFF])


def frames_of(bitrate, packets, n_frames=None):
    return synth.packet_frames(bitrate, [packets], n_frames)


def frames_by_hand(bitrate, per_frame):
    """frames that hold exactly the packets given for each, then padding"""
    rows = []
    for packets in per_frame:
        row = b"".join(packets)
        slots = bitrate // 8
        assert len(row) <= 24 * slots
        while len(row) < 24 * slots:
            row += synth.padding_packet(min(4, slots - len(row) // 24))
        rows.append(np.frombuffer(row, np.uint8))
    return np.stack(rows)


def _streams():
    S = {}
    G = synth.msc_data_group

    def add(name, packets, bitrate=64, **kw):
        counts = kw.pop("counts")
        frames = kw.pop("frames", None)
        S[name] = dict(dict(bitrate=bitrate, frames=frames_of(bitrate, packets) if frames is None else frames, counts=counts), **kw)

    def pk(groups, sizes=(2,), ci=0, address=ADDR):
        return synth.packetise(groups, address, sizes, ci)

    def thin(groups):
        """every group in one-slot packets of at most two useful bytes: at 8 kbit/s a frame holds one of them, so the group, its
        CRC register and its first bytes cross a frame boundary, and with it a call boundary, after every two bytes"""
        out = []
        for g in groups:
            plan = [(1, min(2, len(g) - at)) for at in range(0, len(g), 2)]
            out += synth.packetise_chosen(g, ADDR, plan, ci=len(out))
        return out

    # every header option alone
    alone = [G(0, payload(40, 1), continuity=1), G(1, payload(33, 2), extension=0xBEEF, continuity=2), G(2, payload(50, 3), segment=(5, True), continuity=3),
             G(3, payload(20, 4), user_access=True, end_user=b"abc", continuity=4), G(4, payload(61, 5), tid=0x1234, continuity=5),
             G(5, payload(9, 6), tid=0x0042, end_user=payload(13, 7), continuity=6), G(6, payload(17, 8), user_access=True, end_user=b"", continuity=7),
             G(7, payload(70, 9), continuity=8, repetition=9), G(8, b"", continuity=1)]
    add("every header option alone", pk(alone), counts=dict(groups_emitted=len(alone), groups_closed=len(alone), groups_malformed=0, groups_no_crc=0))
    together = [G(9, payload(100, 10), tid=0xFFFF, segment=(0x7FFF, True), extension=0x8001, end_user=payload(13, 11), continuity=15, repetition=15),
                G(9, payload(3, 12), tid=0, segment=(0, False), extension=0, end_user=b"", continuity=0, crc=False)]
    add("all options together", pk(together, (3, 1)), bitrate=24, counts=dict(groups_emitted=2, groups_no_crc=1))
    add("CRC present, absent, wrong", pk([G(0, payload(30, 13), continuity=1), G(0, payload(31, 14), continuity=2, crc=False),
                                         synth.wrong_crc(G(0, payload(32, 15), continuity=3)), G(0, payload(33, 16), continuity=4)]),
        bitrate=16, counts=dict(groups_emitted=3, groups_no_crc=1, groups_crc_failed=1))
    # headers longer than the group: extension and segment flagged in four bytes, without and with a CRC; three bytes
    short = [bytes([0xA0, 0x10, 1, 2]), with_crc(bytes([0xE0, 0x20, 1, 2])), bytes([0x00, 0x30, 9]), bytes([0x90, 0x40, 0, 0]) + b"\x12",
             with_crc(bytes([0x50, 0x50])), G(0, payload(12, 17), continuity=6)]
    add("a header longer than the group", thin(short), bitrate=8, counts=dict(groups_malformed=5, groups_emitted=1, groups_closed=6))
    li = [bytes([0x10, 0x10, 0x11, 0xAA, 1, 2, 3]), with_crc(bytes([0x50, 0x20, 0x10, 1, 2, 3])), bytes([0x10, 0x30, 0x1F]) + payload(14, 18),
          bytes([0x10, 0x40, 0x12, 0xAB, 0xCD])]
    add("LI below 2 with the transport-id flag", thin(li), bitrate=8, counts=dict(groups_malformed=3, groups_emitted=1))
    # the cap
    exact = G(0, payload(GROUP_CAP - 4, 19), continuity=1)
    more = G(0, payload(GROUP_CAP - 3, 20), continuity=2)
    assert len(exact) == GROUP_CAP and len(more) == GROUP_CAP + 1
    add("a group of exactly 16384 bytes, and one byte more", pk([exact, more, G(1, payload(10, 21), continuity=3)], (4,)), bitrate=512, bytes_capacity=GROUP_CAP + 64,
        counts=dict(groups_too_long=1, groups_emitted=2, packets_orphan=0, bytes_emitted=GROUP_CAP + len(G(1, payload(10, 21)))))
    # shapes of packets
    g = G(3, payload(90, 22), tid=7, continuity=1)
    plan = [(1, 10), (2, 0), (1, 0), (3, 60), (1, 19), (4, 0), (1, len(g) - 89)]
    add("udl 0 packets inside a group", synth.packetise_chosen(g, ADDR, plan) + pk([G(3, payload(5, 23), continuity=2)], ci=len(plan)),
        counts=dict(groups_emitted=2, packets_followed=len(plan) + 1))
    add("a first packet that is also last", pk([G(t, payload(10 + t, 24 + t), continuity=t) for t in range(6)], (1,)), bitrate=8, counts=dict(groups_emitted=6, packets_followed=6))
    plan = [(2, 30), ("command", 1), (2, 30), ("command", 2), (2, len(g) - 60)]
    add("a command packet inside a group", synth.packetise_chosen(g, ADDR, plan), counts=dict(packets_command=2, groups_emitted=1, groups_unfinished=0))
    whole = pk([G(0, payload(200, 30), continuity=1), G(0, payload(20, 31), continuity=2)], (2,))
    add("an orphan run", whole[1:], counts=dict(packets_orphan=len(whole) - 2, groups_emitted=1, continuity_breaks=0))
    three = pk([G(0, payload(200, 32), continuity=1), G(0, payload(200, 33), continuity=2), G(0, payload(20, 34), continuity=3)], (2,))
    per = len(three) // 2
    add("a continuity break inside a group", three[:per + 2] + three[per + 3:], counts=dict(continuity_breaks=1, groups_unfinished=1, groups_emitted=2, packets_orphan=per - 3))
    bad_udl = synth.packet(ADDR, b"x" * 19, 1, ci=2, first=False, last=False, udl=20)
    add("a malformed packet inside a group", three[:2] + [bad_udl] + three[3:], counts=dict(packets_malformed=1, groups_unfinished=1, continuity_breaks=0, groups_emitted=2))
    # repeats
    rep = [G(0, payload(60, 40), continuity=1), G(0, payload(60, 40), continuity=1), G(0, payload(50, 41), continuity=2), G(1, payload(40, 42), continuity=2),
           G(0, payload(50, 41), continuity=2, repetition=1), G(1, payload(40, 43), continuity=3), G(0, payload(50, 44), continuity=1)]
    for keep in (0, 1):
        add("repeats, keep_repeats %d" % keep, pk(rep), keep_repeats=keep, counts=dict(groups_repeated=2, groups_emitted=5 + 2 * keep))
    sixteen = [G(t, payload(20 + t, 50 + t), continuity=(t + r // 2) & 15) for r in range(3) for t in range(16)]
    add("sixteen types interleaved", pk(sixteen), counts=dict(groups_repeated=16, groups_emitted=32))
    # room
    five = [G(0, payload(n, 60 + n), continuity=i + 1) for i, n in enumerate((30, 41, 52, 23, 64))]
    add("max_groups exhausted", pk(five), max_groups=3, cut_visible=True, counts=dict(groups_emitted=3, groups_no_room=2))
    fit = sum((len(x) + 15) // 16 * 16 for x in five[:4]) + len(five[4])
    add("bytes_capacity: an exact fit", pk(five), bytes_capacity=fit, cut_visible=True, counts=dict(groups_emitted=5, groups_no_room=0, bytes_emitted=sum(map(len, five))))
    add("bytes_capacity: one byte short", pk(five), bytes_capacity=fit - 1, cut_visible=True, counts=dict(groups_emitted=4, groups_no_room=1))
    # rates
    small = [G(0, payload(9, 70), continuity=1), G(1, payload(30, 71), tid=5, continuity=1)]
    add("rate 8", pk(small, (1,)), bitrate=8, counts=dict(groups_emitted=2, slots=len(frames_of(8, pk(small, (1,))))))
    big = [G(t & 15, payload(300 + 7 * t, 72 + t), continuity=(t + t // 16) & 15) for t in range(24)]
    add("rate 512", pk(big, (4, 1, 3, 2)), bitrate=512, bytes_capacity=16384, counts=dict(groups_emitted=24))
    # three addresses on one d_in, at 72 kbit/s: two with data groups, one without
    raw = payload(700, 80)
    per = [(ADDR, pk([G(0, payload(80 + i, 81 + i), continuity=i) for i in range(5)], (2, 1)), 0),
           (8, pk([G(2, payload(45 + i, 90 + i), tid=i, continuity=i) for i in range(7)], (1, 3), address=8), 0),
           (9, synth.packetise_raw(raw, 9, (2, 1, 3)), 1)]
    shared = synth.packet_frames(72, [p for _a, p, _m in per])
    for address, packets, mode in per:
        S["shared, address %d" % address] = dict(
            bitrate=72, frames=shared, address=address, mode=mode, share="shared, address %d" % ADDR,
            counts=dict(packets_followed=len(packets), packets_other=sum(len(q) for a, q, _m in per if a != address),
                        **(dict(bytes_emitted=len(raw), groups_emitted=0) if mode else dict(groups_emitted=5 if address == ADDR else 7))))
    # mode 1
    rp = synth.packetise_raw(payload(900, 82), ADDR, (2, 4, 1))
    cmd = synth.packet(ADDR, b"cmd", 1, ci=5, command=True)
    odd = rp[:5] + [cmd] + [synth.packet(ADDR, b"y" * 19, 1, ci=6, udl=21)] + synth.packetise_raw(payload(300, 83), ADDR, (3,), ci=8) + \
        synth.packetise_raw(payload(100, 84), ADDR, (2,), ci=2)
    add("mode 1 with breaks", odd, mode=1, counts=dict(continuity_breaks=2, groups_emitted=2, packets_command=1, packets_malformed=1, bytes_no_room=0, group_bytes=0))
    add("mode 1, capacity exhausted", odd, mode=1, bytes_capacity=400, max_groups=1, cut_visible=True,
        counts=dict(continuity_breaks=2, groups_emitted=1, groups_no_room=1, bytes_emitted=43 + 91 + 19 + 43 + 91 + 67))
    assert all(len(st["frames"]) <= 68 for st in S.values()), {k: len(v["frames"]) for k, v in S.items()}
    return S


def _seams(W):
    """the kernel's own seams: W followed packets make a chunk.  One-slot packets at 512 kbit/s unless said otherwise"""
    S = {}
    G = synth.msc_data_group

    def singles(n, ci, seed):
        """n groups of one packet each"""
        return synth.packetise([G(i & 15, payload(5 + i % 9, seed + i), continuity=((i >> 4) + seed) & 15) for i in range(n)], ADDR, (1,), ci)

    def long_group(n_packets, ci, seed, slots=1, udl=19, dg_type=3):
        g = G(dg_type, payload(n_packets * udl - 4, seed), continuity=9)
        return synth.packetise_chosen(g, ADDR, [(slots, udl)] * n_packets, ci)

    def add(name, packets, **kw):
        counts = kw.pop("counts")
        frames = kw.pop("frames", None)
        S[name] = dict(dict(bitrate=512, frames=frames_of(512, packets) if frames is None else frames, counts=counts, bytes_capacity=1 << 16, max_groups=3 * W), **kw)

    p = singles(2 * W, 0, 100) + long_group(3, 2 * W, 101)
    add("2 W + 3 followed packets", p, counts=dict(packets_followed=2 * W + 3, groups_emitted=2 * W + 1))
    p = singles(W - 1, 0, 110) + long_group(3, W - 1, 111) + singles(2, W + 2, 112)
    add("a group whose first packet is the last of a chunk", p, counts=dict(packets_followed=W + 4, groups_emitted=W + 2))
    p = singles(10, 0, 120) + long_group(2 * W, 10, 121) + singles(3, 2 * W + 10, 122)
    add("a group that opens in chunk 0 and closes in chunk 2", p, counts=dict(packets_followed=2 * W + 13, groups_emitted=14, groups_unfinished=0))
    # W packets of 64 bytes make 16384 exactly when W is 256; the next packet, the first of chunk 1, is one too many
    udl = GROUP_CAP // W
    assert udl * W == GROUP_CAP and udl <= 67
    body = payload(GROUP_CAP + 200, 130)
    over = [synth.packet(ADDR, body[i * udl:(i + 1) * udl], 3, ci=i, first=i == 0, last=False) for i in range(W)] + \
        [synth.packet(ADDR, b"z", 1, ci=W, first=False, last=False), synth.packet(ADDR, b"tail", 1, ci=W + 1, first=False, last=True)] + singles(2, W + 2, 131)
    add("too long exactly at a chunk boundary", over, counts=dict(groups_too_long=1, packets_orphan=1, groups_emitted=2, groups_unfinished=0, group_bytes=GROUP_CAP + sum(
        int(x[2]) & 0x7F for x in singles(2, 0, 131))))
    p = singles(W, 0, 140) + singles(5, W + 1, 141)
    add("a break on the first packet of a chunk, W groups in a chunk", p, counts=dict(continuity_breaks=1, groups_emitted=W + 5, groups_unfinished=0))
    p = singles(30 + 64 * 5, 0, 150)
    rows = [p[:30]] + [p[30 + 64 * i:30 + 64 * (i + 1)] for i in range(5)]
    add("a frame whose 64 followed packets straddle a chunk", None, frames=frames_by_hand(512, rows), counts=dict(packets_followed=350, groups_emitted=350))
    assert all(len(st["frames"]) <= 68 for st in S.values()), {k: len(v["frames"]) for k, v in S.items()}
    return S


_STREAMS, _SEAMS = {}, {}


def streams():
    if not _STREAMS:
        _STREAMS.update(_streams())
    return _STREAMS


def seams():
    if not _SEAMS:
        _SEAMS.update(_seams(dabgpu.packet_groups_chunk()))
    return _SEAMS


STREAM_NAMES = ["every header option alone", "all options together", "CRC present, absent, wrong", "a header longer than the group",
                "LI below 2 with the transport-id flag", "a group of exactly 16384 bytes, and one byte more", "udl 0 packets inside a group",
                "a first packet that is also last", "a command packet inside a group", "an orphan run", "a continuity break inside a group",
                "a malformed packet inside a group", "repeats, keep_repeats 0", "repeats, keep_repeats 1", "sixteen types interleaved", "max_groups exhausted",
                "bytes_capacity: an exact fit", "bytes_capacity: one byte short", "rate 8", "rate 512", "shared, address 7", "shared, address 8",
                "shared, address 9", "mode 1 with breaks", "mode 1, capacity exhausted"]
SEAM_NAMES = ["2 W + 3 followed packets", "a group whose first packet is the last of a chunk", "a group that opens in chunk 0 and closes in chunk 2",
              "too long exactly at a chunk boundary", "a break on the first packet of a chunk, W groups in a chunk",
              "a frame whose 64 followed packets straddle a chunk"]


# ------------------------------------------------------------------------------------------------ running a call
class HostMemory:
    def load(self, img):
        raw = np.empty(img.size + 256, np.uint8)
        off = -raw.ctypes.data % 256
        self.buf = raw[off:off + img.size]
        self.buf[:] = img
        return self.buf.ctypes.data

    def run(self, entries, n_cifs):
        dabgpu.packet_groups_host(entries, n_cifs)

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
        self.ctx.packet_groups_dev(entries, n_cifs)
        self.ctx.sync()

    def read(self):
        self.ctx.sync()
        return self.t.cpu().numpy()


DEFAULTS = dict(address=ADDR, fec=0, mode=0, keep_repeats=0, bytes_capacity=4096, max_groups=64)
KEYS = ("bitrate", "frames", "stride", "in_off", "state") + tuple(DEFAULTS)


def spec_of(st, a=0, b=None, **kw):
    sp = dict(DEFAULTS)
    sp.update({k: v for k, v in st.items() if k in KEYS})
    sp["frames"] = st["frames"][a:b]
    sp.update(kw)
    return sp


def call(mem, specs, n_cifs, mutate=None, refused=None, shared=()):
    """One call on buffers laid out in one allocation, every region between sentinel bytes.  After the call nothing but
    state-out, result, the emitted records and the emitted groups' bytes may have changed (nothing at all for a refused call).
    -> per entry dict(groups [(record, bytes)], stream, result, state)"""
    size, lay = 0, []

    def take(n):
        nonlocal size
        off = (size + GAP + 255) // 256 * 256
        size = off + n
        return off

    nb = dabgpu.packet_groups_state_bytes()
    rb = dabgpu.PACKET_GROUPS_RESULT_DTYPE.itemsize
    for e, sp in enumerate(specs):
        stride = sp.get("stride", 3 * sp["bitrate"])
        frames = lay[shared[e]]["frames"] if e in shared else take(max(n_cifs, 1) * stride + 16) + sp.get("in_off", 0)
        lay.append(dict(frames=frames, sin=take(nb) if sp.get("state") is not None else None, sout=take(nb), bytes=take(max(sp["bytes_capacity"], 1)),
                        groups=take(max(sp["max_groups"], 1) * 32), result=take(rb)))
    img = np.full(size + GAP, FILL, np.uint8)
    for e, (sp, L) in enumerate(zip(specs, lay)):
        stride = sp.get("stride", 3 * sp["bitrate"])
        if e not in shared:
            for k in range(n_cifs):
                img[L["frames"] + k * stride:L["frames"] + k * stride + 3 * sp["bitrate"]] = sp["frames"][k]
        if L["sin"] is not None:
            img[L["sin"]:L["sin"] + nb] = np.frombuffer(bytes(sp["state"]), np.uint8)
    base = mem.load(img)
    assert base % 256 == 0
    entries = [dabgpu.PacketGroupsEntry(base + L["frames"], sp.get("stride", 3 * sp["bitrate"]), sp["bitrate"], sp["address"], sp["fec"], sp["mode"],
                                        sp["keep_repeats"], 0, base + L["sin"] if L["sin"] is not None else None, base + L["sout"],
                                        base + L["bytes"], base + L["groups"], sp["bytes_capacity"], sp["max_groups"], base + L["result"])
               for sp, L in zip(specs, lay)]
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
        res = after[L["result"]:L["result"] + rb].view(dabgpu.PACKET_GROUPS_RESULT_DTYPE)[0]
        untouched[L["result"]:L["result"] + rb] = False
        untouched[L["sout"]:L["sout"] + nb] = False
        n = int(res["groups_emitted"])
        assert 0 <= n <= sp["max_groups"]
        recs = after[L["groups"]:L["groups"] + 32 * n].view(dabgpu.DATA_GROUP_DTYPE)
        untouched[L["groups"]:L["groups"] + 32 * n] = False
        groups, stream = [], b""
        if sp["mode"]:
            m = int(res["bytes_emitted"])
            assert m <= sp["bytes_capacity"]
            stream = after[L["bytes"]:L["bytes"] + m].tobytes()
            untouched[L["bytes"]:L["bytes"] + m] = False
            groups = [(r, b"") for r in recs]
        else:
            for r in recs:
                o, n_bytes = int(r["offset"]), int(r["length"])
                assert 0 <= o and o % 16 == 0 and o + n_bytes <= sp["bytes_capacity"]
                groups.append((r, after[L["bytes"] + o:L["bytes"] + o + n_bytes].tobytes()))
                untouched[L["bytes"] + o:L["bytes"] + o + n_bytes] = False
        out.append(dict(groups=groups, stream=stream, result=res, state=after[L["sout"]:L["sout"] + nb].copy()))
    assert (after[untouched] == img[untouched]).all(), "bytes outside the outputs were written: %s" % np.nonzero(after[untouched] != img[untouched])[0][:8]
    return out


def receiver(sp):
    return R.Receiver(sp["address"], sp["fec"], sp["mode"], sp["keep_repeats"])


def ref_call(rx, sp, n_cifs=None):
    frames = sp["frames"] if n_cifs is None else sp["frames"][:n_cifs]
    out = rx.call(frames, sp["bitrate"], sp["bytes_capacity"], sp["max_groups"])
    out.state = rx.state()
    return out


def explain(got, want):
    bad = {k: (int(got["result"][k]), v) for k, v in want.counts.items() if int(got["result"][k]) != v}
    return " counters (got, want): %s; groups %d / %d" % (bad, len(got["groups"]), len(want.groups))


def same(got, want):
    """emitted records and bytes, the stream, the counters and the state record equal the reference's"""
    if any(int(got["result"][k]) != v for k, v in want.counts.items()) or (got["result"]["reserved"] != 0).any():
        return False
    if len(got["groups"]) != len(want.groups) or got["stream"] != want.stream:
        return False
    for (r, data), (w, wdata) in zip(got["groups"], want.groups):
        if any(int(r[f]) != w[f] for f in R.RECORD_FIELDS) or data != wdata:
            return False
    return state_equals(got["state"], want.state)


def state_equals(raw, want):
    st = raw.view(STATE_DTYPE)[0]
    have = len(want["group"])
    mask = sum(1 << t for t in want["last"])
    last = [want["last"].get(t, 0) for t in range(16)]
    return (int(st["seen"]) == want["seen"] and int(st["prev"]) == want["prev"] and int(st["open"]) == want["open"] and int(st["pad"]) == 0 and
            int(st["have"]) == have and (st["reserved"] == 0).all() and int(st["type_mask"]) == mask and st["last_ci"].tolist() == last and
            st["group"][:have].tobytes() == want["group"] and not st["group"][have:].any() and
            (int(st["crc"]) == (R.P.crc_bit_by_bit(want["group"]) ^ 0xFFFF if want["open"] else 0)))


_WANTED = {}


def wanted(name, table=None):
    """the reference's result of the whole stream in one call: computed once, shared, left unchanged"""
    if name not in _WANTED:
        st = (table or streams())[name]
        sp = spec_of(st)
        _WANTED[name] = ref_call(receiver(sp), sp)
    return _WANTED[name]


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_records_and_sizes(built, tmp_path):
    """the binding against the header: every size and offset a C program prints from include/dabgpu.h"""
    L = dabgpu.lib()
    for name in ("dabgpu_packet_groups_state_bytes", "dabgpu_packet_groups_chunk", "dabgpu_packet_groups_dev", "dabgpu_packet_groups_host",
                 "dabgpu_fig_user_applications"):
        assert hasattr(L, name) and name in dabgpu.EXPORTS
    assert dabgpu.packet_groups_state_bytes() == STATE_DTYPE.itemsize == 32 + GROUP_CAP
    W = dabgpu.packet_groups_chunk()
    assert W >= 64 and W % 64 == 0
    src = tmp_path / "sizes.c"
    fields = {"dabgpu_packet_groups_entry": [f for f, _t in dabgpu.PacketGroupsEntry._fields_],
              "dabgpu_data_group": list(dabgpu.DATA_GROUP_DTYPE.names), "dabgpu_user_application": list(dabgpu.USER_APPLICATION_DTYPE.names),
              "dabgpu_packet_groups_result": ["cifs", "group_bytes", "groups_closed", "bytes_no_room", "reserved"]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dabgpu.h"', "int main(void) {"]
    for s, fs in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for f in fs]
    lines.append('printf("flags %d %d %d %d %d %d %d\\n", DABGPU_DG_EXTENSION, DABGPU_DG_CRC, DABGPU_DG_SEGMENT, DABGPU_DG_USER_ACCESS, '
                 'DABGPU_DG_TRANSPORT_ID, DABGPU_DG_REPEAT, DABGPU_DG_BREAK);')
    lines += ["return 0; }"]
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got["dabgpu_packet_groups_entry"]) == C.sizeof(dabgpu.PacketGroupsEntry)
    for f, _t in dabgpu.PacketGroupsEntry._fields_:
        assert int(got["dabgpu_packet_groups_entry." + f]) == getattr(dabgpu.PacketGroupsEntry, f).offset, f
    for s, dt in (("dabgpu_data_group", dabgpu.DATA_GROUP_DTYPE), ("dabgpu_user_application", dabgpu.USER_APPLICATION_DTYPE),
                  ("dabgpu_packet_groups_result", dabgpu.PACKET_GROUPS_RESULT_DTYPE)):
        assert int(got[s]) == dt.itemsize and dt.itemsize % 8 == 0
        for f in fields[s]:
            assert int(got[s + "." + f]) == dt.fields[f][1], (s, f)
    assert dabgpu.PACKET_GROUPS_RESULT_DTYPE.itemsize % 16 == 0
    assert got["flags"].split() == [str(v) for v in (dabgpu.DG_EXTENSION, dabgpu.DG_CRC, dabgpu.DG_SEGMENT, dabgpu.DG_USER_ACCESS, dabgpu.DG_TRANSPORT_ID,
                                                     dabgpu.DG_REPEAT, dabgpu.DG_BREAK)]
    assert (R.EXTENSION, R.CRC, R.SEGMENT, R.USER_ACCESS, R.TRANSPORT_ID, R.REPEAT, R.BREAK) == (1, 2, 4, 8, 16, 32, 64)


def test_transmit_side_is_what_the_standard_says():
    """the new synth pieces byte by byte: FIG 0/13 (clause 6.3.6), the long form of FIG 0/8, a group in chosen packets"""
    f = synth.fig0_13([(0x1234, 2, [(0x44A, b"\x01\x02"), (0x004, b"")])])
    assert f == bytes([0x0A, 0x0D, 0x12, 0x34, 0x22, 0x89, 0x42, 0x01, 0x02, 0x00, 0x80])
    f = synth.fig0_13([(0xE1234567, 1, [(0x007, b"\xAA")])], pd=1)
    assert f == bytes([0x09, 0x2D, 0xE1, 0x23, 0x45, 0x67, 0x11, 0x00, 0xE1, 0xAA])
    assert synth.fig0_8_long([(0x1234, 3, 0xABC)]) == bytes([0x06, 0x08, 0x12, 0x34, 0x03, 0x8A, 0xBC])
    g = synth.msc_data_group(5, b"0123456789", continuity=3)
    p = synth.packetise_chosen(g, 9, [(1, 4), ("command", 1), (2, 0), (1, len(g) - 4)], ci=2)
    assert [len(x) for x in p] == [24, 24, 48, 24]
    assert [(x[0] >> 4) & 3 for x in p] == [2, 3, 0, 1] and [(x[0] >> 2) & 3 for x in p] == [2, 3, 0, 1]
    assert [x[2] for x in p] == [4, 0x83, 0, len(g) - 4] and p[0][3:7] + p[3][3:3 + len(g) - 4] == g
    raw = synth.packetise_raw(b"r" * 100, 9, (1, 2))
    assert b"".join(x[3:3 + (x[2] & 0x7F)] for x in raw) == b"r" * 100 and [x[2] for x in raw] == [19, 43, 19, 19]
    assert synth.wrong_crc(g)[:-1] == g[:-1] and synth.wrong_crc(g) != g


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_host_equals_the_reference(built, name):
    """each stream in one call: the reference itself reports what the stream is about; then records, bytes, counters and the
    state record of the host twin equal the reference's"""
    st = streams()[name]
    want = wanted(name)
    for key, value in st["counts"].items():
        assert want.counts[key] == value, (name, key, want.counts[key], value)
    got = call(HostMemory(), [spec_of(st)], len(st["frames"]))[0]
    assert same(got, want), name + explain(got, want)


@pytest.mark.parametrize("name", SEAM_NAMES)
def test_host_equals_the_reference_on_the_seam_streams(built, name):
    st = seams()[name]
    want = wanted(name, seams())
    for key, value in st["counts"].items():
        assert want.counts[key] == value, (name, key, want.counts[key], value)
    got = call(HostMemory(), [spec_of(st)], len(st["frames"]))[0]
    assert same(got, want), name + explain(got, want)


def joined(outs, mode):
    """the emissions of consecutive calls as one: (record fields but offset and cif, bytes) per group"""
    keys = [f for f in R.RECORD_FIELDS if f not in ("offset", "cif")]
    if outs and isinstance(outs[0], dict):
        groups = [(tuple(int(r[f]) for f in keys), d) for o in outs for r, d in o["groups"]]
        return groups, b"".join(o["stream"] for o in outs)
    return [(tuple(w[f] for f in keys), d) for o in outs for w, d in o.groups], b"".join(o.stream for o in outs)


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_cut_into_two_calls_at_every_frame_boundary(built, name):
    """each stream cut into two calls at EVERY frame boundary, the state handed on: groups, their CRC registers and the repeat
    memory span the calls.  Every call equals the reference's call on the same frames; the joined emissions, the summed
    counters and the last state equal the uncut run, unless a per-call cap makes the cut visible (the reference decides)"""
    st = streams()[name]
    n = len(st["frames"])
    whole = wanted(name)
    assert n >= 2, "a stream of one frame has no boundary to cut at"
    for cut in range(1, n):
        rx, state, gots, wants = receiver(spec_of(st)), None, [], []
        for a, b in ((0, cut), (cut, n)):
            sp = spec_of(st, a, b, state=state)
            want = ref_call(rx, sp)
            got = call(HostMemory(), [sp], b - a)[0]
            assert same(got, want), "%s cut at %d, frames %d..%d:%s" % (name, cut, a, b, explain(got, want))
            state = got["state"]
            gots.append(got)
            wants.append(want)
        if not st.get("cut_visible"):
            sums = R.total(wants)
            assert all(sums[k] == whole.counts[k] for k in R.COUNTERS), (name, cut)
            if not st.get("mode"):
                assert joined(gots, 0)[0] == joined([whole], 0)[0], (name, cut)
            else:
                assert joined(gots, 1)[1] == whole.stream, (name, cut)
            assert state_equals(state, whole.state), (name, cut)


def test_a_repeat_whose_original_closed_in_an_earlier_call(built):
    st = streams()["repeats, keep_repeats 1"]
    n = len(st["frames"])
    seen = 0
    for cut in range(1, n):
        rx = receiver(spec_of(st))
        first = ref_call(rx, spec_of(st, 0, cut))
        second = ref_call(rx, spec_of(st, cut, n))
        if second.groups and second.groups[0][0]["flags"] & R.REPEAT and first.groups:
            seen += 1
            a = call(HostMemory(), [spec_of(st, 0, cut)], cut)[0]
            b = call(HostMemory(), [spec_of(st, cut, n, state=a["state"])], n - cut)[0]
            assert int(b["groups"][0][0]["flags"]) & dabgpu.DG_REPEAT and same(b, second)
    assert seen >= 1


def test_a_foreign_or_corrupted_state_record_is_a_fresh_start(built):
    name = "repeats, keep_repeats 0"
    st = streams()[name]
    n = len(st["frames"])
    fresh = wanted(name)
    nb = dabgpu.packet_groups_state_bytes()
    rng = np.random.default_rng(5)
    good = call(HostMemory(), [spec_of(st, 0, 2)], 2)[0]["state"]
    assert good.view(STATE_DTYPE)[0]["seen"] == 1
    records = [rng.integers(0, 256, nb, dtype=np.uint8), np.full(nb, 0xFF, np.uint8)]
    for field, value in (("seen", 2), ("prev", 4), ("open", 2), ("pad", 1), ("have", GROUP_CAP + 1), ("reserved", 1), ("last_ci", 16)):
        bad = good.copy()
        v = bad.view(STATE_DTYPE)
        if field in ("reserved", "last_ci"):
            v[field][0][3] = value
            if field == "last_ci":
                v["type_mask"][0] |= 8
        else:
            v[field][0] = value
        records.append(bad)
    bad = good.copy()                                                  # a continuity index of a type the mask does not name
    bad.view(STATE_DTYPE)["last_ci"][0][15] = 3
    bad.view(STATE_DTYPE)["type_mask"][0] &= 0x7FFF
    records.append(bad)
    bad = np.zeros(nb, np.uint8)                                       # bytes of a group that is not open
    bad.view(STATE_DTYPE)["have"][0] = 5
    records.append(bad)
    for rec in records:
        got = call(HostMemory(), [spec_of(st, state=rec)], n)[0]
        assert same(got, fresh), explain(got, fresh)
    # garbage in the group buffer behind `have` is not carried on, and a record with an open group of 16384 bytes is taken
    tail = good.copy()
    tail.view(STATE_DTYPE)["group"][0][int(tail.view(STATE_DTYPE)["have"][0]):] = 0x5A
    a = call(HostMemory(), [spec_of(st, 2, n, state=tail)], n - 2)[0]
    b = call(HostMemory(), [spec_of(st, 2, n, state=good)], n - 2)[0]
    assert a["state"].tobytes() == b["state"].tobytes() and (a["result"] == b["result"])
    full = np.zeros(nb, np.uint8)
    v = full.view(STATE_DTYPE)
    v["seen"][0], v["open"][0], v["have"][0], v["prev"][0] = 1, 1, GROUP_CAP, 3
    got = call(HostMemory(), [spec_of(st, state=full)], n)[0]
    assert int(got["result"]["groups_unfinished"]) == fresh.counts["groups_unfinished"] + 1


def refusal_specs():
    st = streams()["every header option alone"]
    n = len(st["frames"])
    return [spec_of(st, state=np.zeros(dabgpu.packet_groups_state_bytes(), np.uint8)), spec_of(streams()["mode 1 with breaks"])], min(n, 8)


def _set(field, value, e=1):
    return lambda entries: setattr(entries[e], field, value(entries[e]) if callable(value) else value)


BAD_ENTRIES = [(_set("bitrate_kbps", 0), ARG), (_set("bitrate_kbps", 520), ARG), (_set("bitrate_kbps", 60), ARG), (_set("in_stride", 10), ARG),
               (_set("address", 0), ARG), (_set("address", 1024), ARG), (_set("d_in", None), ARG), (_set("mode", 2), ARG), (_set("mode", -1), ARG),
               (_set("d_state_out", None), ARG), (_set("d_result", None), ARG), (_set("d_state_out", lambda e: e.d_state_out + 8), ARG),
               (_set("d_state_in", lambda e: e.d_state_out + 16, 0), ARG), (_set("d_state_in", lambda e: e.d_state_in + 4, 0), ARG),
               (_set("d_bytes", lambda e: e.d_bytes + 8), ARG), (_set("d_bytes", None), ARG), (_set("d_groups", None), ARG),
               (_set("d_groups", lambda e: e.d_groups + 2), ARG), (_set("d_result", lambda e: e.d_result + 2), ARG), (_set("bytes_capacity", -1), ARG),
               (_set("max_groups", -1), ARG)]


def test_refused_calls_leave_every_output_alone(built):
    specs, n = refusal_specs()
    for m, code in BAD_ENTRIES:
        call(HostMemory(), specs, n, mutate=m, refused=code)
    L = dabgpu.lib()
    assert L.dabgpu_packet_groups_host(None, 1, 1) == ARG and L.dabgpu_packet_groups_host(None, -1, 1) == ARG
    assert L.dabgpu_packet_groups_host(None, 0, 1) == 0 and L.dabgpu_packet_groups_dev(None, None, 0, 0, None) == ARG
    e = dabgpu.PacketGroupsEntry(1 << 20, 1536, 512, 1, 0, 0, 0, 0, None, 1 << 21, None, None, 0, 0, 1 << 22)
    arr = (dabgpu.PacketGroupsEntry * 1)(e)
    assert L.dabgpu_packet_groups_host(arr, 1, (1 << 31) // 1536 + 1) == CAPACITY and L.dabgpu_packet_groups_host(arr, 1, (1 << 24) + 1) == ARG
    # NULL outputs go with zero capacities
    st = streams()["sixteen types interleaved"]
    got = call(HostMemory(), [spec_of(st, bytes_capacity=0, max_groups=0)], len(st["frames"]),
               mutate=lambda entries: (setattr(entries[0], "d_bytes", None), setattr(entries[0], "d_groups", None)))[0]
    assert int(got["result"]["groups_no_room"]) == 32 and int(got["result"]["groups_emitted"]) == 0


# ---- FIG 0/13
def fic_streams():
    F = {}
    base = [synth.fig0_1([dict(id=5, start=0, option=0, level=3, size=24), dict(id=9, start=100, option=0, level=3, size=48)]),
            synth.fig0_2([dict(sid=0x1111, components=[dict(subchannel=5, ascty=63)]), dict(sid=0x2222, components=[dict(scid=0x123), dict(scid=0x456, primary=False)])]),
            synth.fig0_3([dict(scid=0x123, subchannel=9, address=7, dscty=5), dict(scid=0x456, subchannel=9, address=300, dscty=60, caorg=0xAAAA)])]
    g8 = [synth.fig0_8([(0x1111, 0, 5)]), synth.fig0_8_long([(0x2222, 0, 0x123), (0x2222, 1, 0x456)])]
    g13 = [synth.fig0_13([(0x1111, 0, [(0x002, b"\x0c\x3c")]), (0x2222, 0, [(0x44A, b"\x00"), (0x004, b"tpeg")])]),
           synth.fig0_13([(0x2222, 1, [(0x007, b"")]), (0x2222, 0, [(0x44A, b"again")])])]
    F["both joins"] = (base + g8 + g13, None, 4)
    F["an application before its FIG 0/8"] = (g13 + base + g8, None, 4)
    F["P/D 1"] = (base + [synth.fig0_8_long([(0xE0222222, 2, 0x123)], pd=1), synth.fig0_13([(0xE0222222, 2, [(0x00D, payload(21, 1))])], pd=1)], None, 1)
    F["no FIG 0/8, no FIG 0/3"] = ([synth.fig0_13([(0x3333, 4, [(0x7FF, payload(23, 2))])]), synth.fig0_8_long([(0x4444, 0, 0x789)]), synth.fig0_13([(0x4444, 0, [(1, b"")])])], None, 2)
    F["a FIB with a bad CRC"] = (base + g8 + g13, "last", 3)
    F["other configurations are ignored"] = (base + g8 + [synth.fig0(13, synth.fig0_13([(0x1111, 0, [(2, b"")])])[2:], cn=1), synth.fig0(13, synth.fig0_13([(0x1111, 0, [(3, b"")])])[2:], oe=1),
                                                          synth.fig0_13([(0x1111, 0, [(4, b"")])])], None, 1)
    # FIG 0/8 short form with the MSC/FIC flag set (a FIDC) is passed over: the proper entry behind it makes the join
    fidc = synth.fig0(8, bytes([0x11, 0x11, 0x00, 0x45]))
    F["a FIDC entry of FIG 0/8 is passed over"] = (base + [fidc] + g8 + g13, None, 4)
    F["a FIDC entry alone joins nothing"] = (base + [fidc, synth.fig0_13([(0x1111, 0, [(0x002, b"")])])], None, 1)
    F["cut off by the end of the FIG"] = ([bytes([0x07, 0x0D, 0x55, 0x55, 0x02, 0x00, 0x40, 0x00, 0x9F])], None, 1)
    return F


def fibs_of(figs, spoil):
    fibs = synth.pack_fibs(figs)
    n_frames = -(-len(fibs) // 12)
    fib = np.zeros((n_frames * 12, 32), np.uint8)
    fib[:, 0] = 0xFF
    fib[:len(fibs)] = fibs
    ok = np.zeros(n_frames * 12, np.uint8)
    ok[:len(fibs)] = 1
    if spoil == "last":
        ok[len(fibs) - 1] = 0
    return fib.reshape(n_frames, 12, 32), ok.reshape(n_frames, 12)


@pytest.mark.parametrize("name", list(fic_streams()))
def test_user_applications_equal_the_reference(built, name):
    figs, spoil, count = fic_streams()[name]
    fib, ok = fibs_of(figs, spoil)
    want = R.user_applications(fib, ok)
    assert len(want) == count, (name, want)
    got = dabgpu.fig_user_applications(fib, ok)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for key in ("sid", "scids", "ua_type", "tmid_packet", "subchid", "scid", "packet_address"):
            assert int(g[key]) == w[key], (name, key, g, w)
        n = int(g["data_length"])
        assert g["data"][:n].tobytes() == w["data"] and not g["data"][n:].any() and int(g["reserved"]) == 0
    if name.startswith("a FIDC entry"):
        first = [w for w in want if w["sid"] == 0x1111][0]
        assert first["subchid"] == (5 if "passed over" in name else -1) and first["tmid_packet"] == 0
    if name == "both joins":
        by = {(w["sid"], w["scids"], w["ua_type"]): w for w in want}
        assert by[(0x1111, 0, 2)]["subchid"] == 5 and by[(0x1111, 0, 2)]["tmid_packet"] == 0
        assert by[(0x2222, 0, 0x44A)]["data"] == b"\x00" and by[(0x2222, 0, 0x44A)]["packet_address"] == 7
        assert by[(0x2222, 1, 7)]["packet_address"] == 300 and by[(0x2222, 1, 7)]["subchid"] == 9
        # capacity: nothing written
        out = np.full(4, 0x5A5A5A5A, np.uint32).view(np.uint8).repeat(14)[:4 * 56].copy()
        n_out = C.c_int(0)
        rc = dabgpu.lib().dabgpu_fig_user_applications(fib.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p), fib.shape[0],
                                                       out.ctypes.data_as(C.c_void_p), 3, C.byref(n_out))
        assert rc == CAPACITY and n_out.value == 4 and (out == 0x5A).all()
        assert dabgpu.lib().dabgpu_fig_user_applications(None, None, 1, None, 0, C.byref(n_out)) == ARG


# ---- device code
def test_the_kernel_neither_spills_nor_uses_scratch(built, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the device assembly cannot be checked")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "packet_groups_kernels.hip" in mk
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    out = tmp_path / "packet_groups_kernels.s"
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "packet_groups_kernels.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    md = kernel_metadata(out.read_text())
    assert len(md) == 1 and all("packet_groups_kernel" in k for k in md)
    for k, v in md.items():
        print("%s: vgprs %s, LDS %s bytes" % (k, v.get("vgpr_count"), v.get("group_segment_fixed_size")))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["group_segment_fixed_size"] <= 48 * 1024


def test_the_walk_under_sanitizers_on_random_frames_and_state_records(built, tmp_path):
    """tests/packet_groups_fuzz.cpp: include/dabgpu_data_groups.h's serial walk on random and mutated frames and random state
    records, every buffer a heap block of exactly its size; a stand-alone program built with the host compiler under
    AddressSanitizer and UBSan and run as a child process"""
    exe = str(tmp_path / "packet_groups_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "packet_groups_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "4000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "calls=4000" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = dict(kv.split("=") for kv in r.stdout.split())
    for key in ("groups_emitted", "groups_crc_failed", "groups_malformed", "groups_repeated", "groups_too_long", "groups_no_room", "continuity_breaks",
                "bytes_no_room", "fresh_starts", "carried_open"):
        assert int(got[key]) > 0, (key, r.stdout)


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


def all_specs(names=STREAM_NAMES, table=None, n_cifs=None):
    """every stream as one entry of one table: in_stride beyond the frame and frames off their 16-byte and 4-byte boundaries by
    turns, the three entries of the shared sub-channel naming the same frames"""
    specs, shared, index = [], {}, {}
    for e, name in enumerate(names):
        st = (table or streams())[name]
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


def held(pctx, specs, n, names, shared=()):
    wants = [ref_call(receiver(sp), sp, n) for sp in specs]
    got = call(DeviceMemory(pctx), specs, n, shared=shared)
    host = call(HostMemory(), specs, n, shared=shared)
    for name, g, h, w in zip(names, got, host, wants):
        assert same(g, w), str(name) + explain(g, w)
        assert same(h, w), name
        assert g["state"].tobytes() == h["state"].tobytes() and g["result"].tobytes() == h["result"].tobytes(), name
    return got


@pytest.mark.gpu
def test_gpu_every_stream_in_one_call(pctx):
    """all streams in ONE call of 68 logical frames (rows of 0xFF behind the shorter streams): bit rates 8, 64, 72 and 512,
    both modes, three entries on one d_in, in_stride beyond 3 R, d_in off 16 and off 4 bytes: records, bytes, counters and the
    state record equal the reference and the host call"""
    specs, shared = all_specs()
    got = held(pctx, padded(specs, 68), 68, STREAM_NAMES, shared)
    assert sum(len(g["groups"]) for g in got) == sum(streams()[n]["counts"]["groups_emitted"] for n in STREAM_NAMES) >= 100


@pytest.mark.gpu
@pytest.mark.parametrize("n_cifs", [0, 1, 7])
def test_gpu_short_calls(pctx, n_cifs):
    """calls of 0, 1 and 7 logical frames (68 is the call above), every entry"""
    specs, shared = all_specs()
    held(pctx, padded(specs, 7), n_cifs, STREAM_NAMES, shared)


@pytest.mark.gpu
def test_gpu_the_seams_of_the_kernel(pctx):
    """W followed packets make a chunk: 2 W + 3 packets; a group whose first packet is the last of a chunk; one that opens in
    chunk 0 and closes in chunk 2; the too-long threshold crossed by the first packet of a chunk; a break on the first packet
    of a chunk; W groups in one chunk; a frame whose 64 packets straddle a chunk"""
    for name in SEAM_NAMES:
        want = wanted(name, seams())
        for key, value in seams()[name]["counts"].items():
            assert want.counts[key] == value, (name, key)
    specs, shared = all_specs(SEAM_NAMES, seams())
    held(pctx, padded(specs, 20), 20, SEAM_NAMES, shared)


@pytest.mark.gpu
def test_gpu_130_entries_in_one_table(pctx):
    """130 entries: thirteen streams of at most 24 frames, ten times over with modes, rates and capacities mixed, each with
    outputs of its own"""
    names = ["every header option alone", "all options together", "CRC present, absent, wrong", "a header longer than the group",
             "udl 0 packets inside a group", "a command packet inside a group", "a continuity break inside a group", "repeats, keep_repeats 0",
             "sixteen types interleaved", "rate 8", "rate 512", "mode 1 with breaks", "mode 1, capacity exhausted"]
    assert all(len(streams()[n]["frames"]) <= 24 for n in names)
    assert len(names) == 13 and len({streams()[n]["bitrate"] for n in names}) >= 2 and any(streams()[n].get("mode") for n in names)
    specs, labels = [], []
    for rep in range(10):
        for i, name in enumerate(names):
            st = streams()[name]
            sp = spec_of(st, stride=3 * st["bitrate"] + (rep + i) % 7, in_off=(3 * rep + i) % 16)
            if rep % 3 == 1:
                sp.update(bytes_capacity=[0, 48, 100, 333][(rep + i) % 4])
            if rep % 3 == 2:
                sp.update(max_groups=[0, 1, 2, 5][(rep + i) % 4], keep_repeats=1)
            specs.append(sp)
            labels.append((rep, name))
    assert len(specs) == 130
    held(pctx, padded(specs, 24), 24, labels)


@pytest.mark.gpu
def test_gpu_two_calls_back_to_back_with_the_state_on_the_device(pctx):
    """streams in two calls enqueued one behind the other, nothing waiting in between: the state record of the first is the
    second's input.  The cuts lie inside a group (its bytes and its CRC register span the calls; the 16384-byte one among
    them) and between a group and its repeat"""
    import torch
    names = ["a group of exactly 16384 bytes, and one byte more", "repeats, keep_repeats 1", "udl 0 packets inside a group", "sixteen types interleaved",
             "mode 1 with breaks", "rate 512"]
    nb, rb = dabgpu.packet_groups_state_bytes(), dabgpu.PACKET_GROUPS_RESULT_DTYPE.itemsize
    bufs, wants, cuts = [], [], []
    for name in names:
        st = streams()[name]
        n = len(st["frames"])
        cut = {"a group of exactly 16384 bytes, and one byte more": 5, "repeats, keep_repeats 1": 2}.get(name, n // 2)
        sp = spec_of(st)
        rx = receiver(sp)
        first = ref_call(rx, spec_of(st, 0, cut))
        second = ref_call(rx, spec_of(st, cut, n))
        assert first.state["open"] or name.startswith(("sixteen", "mode 1")), name
        assert not name.startswith("repeats") or second.groups[0][0]["flags"] & R.REPEAT
        wants.append((first, second))
        cuts.append((cut, n))
        t = dict(frames=torch.from_numpy(np.ascontiguousarray(st["frames"])).cuda(), state=torch.full((2, nb), FILL, dtype=torch.uint8, device="cuda"),
                 bytes=torch.full((2, sp["bytes_capacity"]), FILL, dtype=torch.uint8, device="cuda"),
                 groups=torch.full((2, sp["max_groups"] * 32), FILL, dtype=torch.uint8, device="cuda"),
                 result=torch.full((2, rb), FILL, dtype=torch.uint8, device="cuda"))
        bufs.append((sp, t))
    # (one call per stream and half: the frames of a call are n_cifs for all its entries)
    torch.cuda.synchronize()
    for (sp, t), (cut, n) in zip(bufs, cuts):
        row = 3 * sp["bitrate"]
        for half, (a, b) in enumerate(((0, cut), (cut, n))):
            e = dabgpu.PacketGroupsEntry(t["frames"].data_ptr() + a * row, row, sp["bitrate"], sp["address"], sp["fec"], sp["mode"], sp["keep_repeats"], 0,
                                         t["state"][0].data_ptr() if half else None, t["state"][half].data_ptr(), t["bytes"][half].data_ptr(),
                                         t["groups"][half].data_ptr(), sp["bytes_capacity"], sp["max_groups"], t["result"][half].data_ptr())
            pctx.packet_groups_dev([e], b - a)
    pctx.sync()
    for name, (sp, t), pair in zip(names, bufs, wants):
        for half, want in enumerate(pair):
            res = t["result"][half].cpu().numpy().view(dabgpu.PACKET_GROUPS_RESULT_DTYPE)[0]
            recs = t["groups"][half].cpu().numpy()[:32 * int(res["groups_emitted"])].view(dabgpu.DATA_GROUP_DTYPE)
            data = t["bytes"][half].cpu().numpy()
            if sp["mode"]:
                got = dict(groups=[(r, b"") for r in recs], stream=data[:int(res["bytes_emitted"])].tobytes(), result=res, state=t["state"][half].cpu().numpy())
            else:
                got = dict(groups=[(r, data[int(r["offset"]):int(r["offset"]) + int(r["length"])].tobytes()) for r in recs], stream=b"", result=res,
                           state=t["state"][half].cpu().numpy())
            assert same(got, want), "%s, call %d:%s" % (name, half, explain(got, want))


@pytest.mark.gpu
def test_gpu_refused_calls_leave_every_output_alone(pctx):
    specs, n = refusal_specs()
    for m, code in BAD_ENTRIES:
        call(DeviceMemory(pctx), specs, n, mutate=m, refused=code)


# ---- more frames than the kernel takes at a time
def long_call_stream():
    """8 kbit/s: one one-slot packet a frame, W + 30 frames, so the kernel's frame loop runs twice; a group of 30 packets lies
    across the seam between its two blocks of W frames"""
    W = dabgpu.packet_groups_chunk()
    G = synth.msc_data_group
    first = synth.packetise([G(i & 15, payload(5 + i % 9, 500 + i), continuity=(i >> 4) & 15) for i in range(W - 10)], ADDR, (1,))
    across = synth.packetise_chosen(G(5, payload(30 * 19 - 4, 499), continuity=7), ADDR, [(1, 19)] * 30, ci=W - 10)
    last = synth.packetise([G(i & 15, payload(6 + i, 800 + i), continuity=9) for i in range(10)], ADDR, (1,), ci=W + 20)
    frames = frames_of(8, first + across + last)
    assert len(frames) == W + 30
    return dict(bitrate=8, frames=frames, max_groups=W + 30, bytes_capacity=1 << 16, counts=dict(packets_followed=W + 30, groups_emitted=W + 1, groups_unfinished=0))


def test_host_equals_the_reference_on_more_frames_than_a_block(built):
    st = long_call_stream()
    sp = spec_of(st)
    want = ref_call(receiver(sp), sp)
    for key, value in st["counts"].items():
        assert want.counts[key] == value, (key, want.counts[key], value)
    got = call(HostMemory(), [sp], len(st["frames"]))[0]
    assert same(got, want), explain(got, want)


@pytest.mark.gpu
def test_gpu_more_frames_than_a_block(pctx):
    """the kernel takes the scan records of W frames at a time: W + 30 frames, a group across the seam, beside an entry of
    another rate that ends within the first block"""
    st = long_call_stream()
    n = len(st["frames"])
    other = streams()["rate 512"]
    specs = padded([spec_of(st, stride=24 + 3, in_off=5), spec_of(other)], n)
    held(pctx, specs, n, ["W + 30 frames", "rate 512 beside it"])


# ---- end to end
E2E_SEED = 4
E2E_DABPLUS = [("Radio One", 0xC221, 3, 0, 3, 64, 0)]
E2E_SID, E2E_SUBCH, E2E_START = 0xD302, 9, 48
E2E_COMPONENTS = [(0x123, ADDR, 5, 0), (0x124, 8, 5, 1)]            # (SCId, packet address, DSCTy, DG flag)
E2E_APPS = [(E2E_SID, 0, 0x123, [(0x004, b"\x01")]), (E2E_SID, 1, 0x124, [(0x44A, b"")])]
E2E_RAW = payload(300, 301)


def e2e_groups():
    G = synth.msc_data_group
    return [G(0, payload(35, 302), continuity=1), G(4, payload(30, 303), tid=0x77, segment=(0, False), continuity=1),
            G(0, payload(33, 304), continuity=2), G(4, payload(28, 305), tid=0x77, segment=(1, True), continuity=2)]


def e2e_ensemble():
    """one ensemble: a DAB+ service of 64 kbit/s, and a packet-mode sub-channel of 32 kbit/s with two components: address 7
    sends a mix of type-0 and type-4 data groups, each twice in a row (the second a repeat), address 8 a byte string without
    data groups; a cycle of 20 logical frames"""
    twice = [g for g in e2e_groups() for _ in range(2)]
    pk = synth.packetise(twice, ADDR, sizes=(2,))
    raw = synth.packetise_raw(E2E_RAW, 8, (1,))
    assert all(len(g) <= 43 for g in twice) and len(pk) % 4 == 0 and len(raw) % 4 == 0      # (the continuity index goes on where the cycle wraps)
    frames = synth.packet_frames(32, [pk, raw], n_frames=20)
    assert frames.shape == (20, 96), frames.shape
    service = ("Data", E2E_SID, E2E_SUBCH, 0, 3, 32, E2E_START, E2E_COMPONENTS, frames, 0)
    return synth.ServiceEnsemble(E2E_SEED, E2E_DABPLUS, n_frames=5, extras=False, packet_services=[service], user_applications=E2E_APPS), frames


def test_end_to_end_multiplex_carries_the_groups(built):
    """what the GPU test will receive: the FIC's components and user applications, and the reference receiver on the
    transmitted logical frames, two cycles of them"""
    ens, frames = e2e_ensemble()
    ok = np.ones((5, 12), np.uint8)
    comps = dabgpu.fig_packet_components(ens.fibs, ok)
    assert [(c.subchid, c.packet_address, c.dscty, c.dg_flag) for c in comps] == [(E2E_SUBCH, ADDR, 5, 0), (E2E_SUBCH, 8, 5, 1)]
    apps = dabgpu.fig_user_applications(ens.fibs, ok)
    assert [(int(a["ua_type"]), int(a["tmid_packet"]), int(a["subchid"]), int(a["packet_address"])) for a in apps] == \
        [(dabgpu.UA_TPEG, 1, E2E_SUBCH, ADDR), (dabgpu.UA_JOURNALINE, 1, E2E_SUBCH, 8)]
    assert [{k: (int(a[k]) if k != "data" else a["data"][:int(a["data_length"])].tobytes()) for k in w} for a, w in zip(apps, R.user_applications(ens.fibs, ok))] == \
        R.user_applications(ens.fibs, ok)
    two = np.concatenate([frames, frames])
    out = R.Receiver(ADDR).call(two, 32, 4096, 64)
    assert [d for _r, d in out.groups] == e2e_groups() * 2 and out.counts["groups_repeated"] == 8 and out.counts["slots_bad"] == 0
    raw = R.Receiver(8, 0, 1).call(two, 32, 4096, 64)
    assert raw.stream == E2E_RAW * 2 and raw.counts["continuity_breaks"] == 0


@pytest.mark.gpu
def test_gpu_end_to_end_iq_to_groups(pctx):
    """IQ of 16 transmission frames of that ensemble -> front end -> FIC pass -> fig_subchannels, fig_packet_components and
    fig_user_applications -> decode_ensembles_dev -> packet_groups_dev behind it on the same stream, nothing waiting in
    between: every group exactly once (its repetition held back), the raw bytes of the other component, and not one packet lost"""
    import torch
    dev = torch.device("cuda", 0)
    fps, L, FB = 16, 76 * 2552, dabgpu.NB_FRAME_BITS
    ens, frames = e2e_ensemble()
    tx = ens.iq()
    c = pctx
    c.streams_reset(1)
    rx = synth.channel(tx[np.arange(fps) % 5].ravel(), snr_db=20.0, rng=np.random.default_rng(13)).reshape(fps, -1)
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
    comps = dabgpu.fig_packet_components(fib_h, ok_h)
    apps = dabgpu.fig_user_applications(fib_h, ok_h)
    assert [sc.bitrate_kbps for sc in plan] == [64, 32] and len(comps) == 2 and len(apps) == 2
    # the application says what the data is for, the component how it is sent: joined by (SubChId, packet address)
    chosen = []
    for a in apps:
        comp = [q for q in comps if (q.subchid, q.packet_address) == (int(a["subchid"]), int(a["packet_address"]))]
        assert len(comp) == 1 and int(a["tmid_packet"]) == 1 and int(a["scid"]) == comp[0].scid
        chosen.append((int(a["ua_type"]), comp[0]))
    assert [(t, q.packet_address, q.dg_flag) for t, q in chosen] == [(dabgpu.UA_TPEG, ADDR, 0), (dabgpu.UA_JOURNALINE, 8, 1)]
    j = [sc.start_address for sc in plan].index(comps[0].start_address)
    br, n_cifs = plan[j].bitrate_kbps, 4 * fps
    hist = [torch.zeros((15, sc.length * 64), dtype=torch.int8, device=dev) for sc in plan]
    outs = [torch.zeros((n_cifs, sc.bitrate_kbps * 3), dtype=torch.uint8, device=dev) for sc in plan]
    nb, rb, cap, mg = dabgpu.packet_groups_state_bytes(), dabgpu.PACKET_GROUPS_RESULT_DTYPE.itemsize, 4096, 64
    state = torch.zeros((2, nb), dtype=torch.uint8, device=dev)
    data = torch.full((2, cap), FILL, dtype=torch.uint8, device=dev)
    recs = torch.full((2, mg * 32), FILL, dtype=torch.uint8, device=dev)
    result = torch.zeros((2, rb), dtype=torch.uint8, device=dev)
    c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), [plan], None, [[h.data_ptr() for h in hist]],
                           [[o.data_ptr() for o in outs]], None)
    # (the time de-interleaver starts empty: the first 15 logical frames of a sub-channel are not decodable, whatever follows
    # them; the call is given the frames from the 16th on, and on those not one packet may be lost)
    skip = 16
    c.packet_groups_dev([dabgpu.PacketGroupsEntry(outs[j].data_ptr() + skip * 3 * br, 3 * br, br, q.packet_address, q.fec_scheme, q.dg_flag, 0, 0, None,
                                                  state[e].data_ptr(), data[e].data_ptr(), recs[e].data_ptr(), cap, mg, result[e].data_ptr())
                         for e, (_t, q) in enumerate(chosen)], n_cifs - skip)
    c.sync()                                                          # (the only wait behind the decode call)
    decoded = outs[j].cpu().numpy()[skip:]
    for e, (_t, q) in enumerate(chosen):
        rx = R.Receiver(q.packet_address, q.fec_scheme, q.dg_flag, 0)
        want = rx.call(decoded, br, cap, mg)
        want.state = rx.state()
        assert want.counts["slots_bad"] == 0 and want.counts["continuity_breaks"] == 0 and want.counts["groups_crc_failed"] == 0, want.counts
        res = result[e].cpu().numpy().view(dabgpu.PACKET_GROUPS_RESULT_DTYPE)[0]
        rr = recs[e].cpu().numpy()
        got_recs = rr[:32 * int(res["groups_emitted"])].view(dabgpu.DATA_GROUP_DTYPE)
        raw = data[e].cpu().numpy()
        assert (rr[32 * int(res["groups_emitted"]):] == FILL).all()
        if q.dg_flag:
            got = dict(groups=[(r, b"") for r in got_recs], stream=raw[:int(res["bytes_emitted"])].tobytes(), result=res, state=state[e].cpu().numpy())
            assert (raw[int(res["bytes_emitted"]):] == FILL).all() and len(got["stream"]) >= 2 * len(E2E_RAW)
            both = E2E_RAW * 4
            assert got["stream"] in both
        else:
            got = dict(groups=[(r, raw[int(r["offset"]):int(r["offset"]) + int(r["length"])].tobytes()) for r in got_recs], stream=b"", result=res,
                       state=state[e].cpu().numpy())
            # every group exactly once: the cycle's four groups in their order, again and again, and as many repeats held back
            sent_groups = [d for _r, d in got["groups"]]
            cyc = e2e_groups()
            first = cyc.index(sent_groups[0])
            assert len(sent_groups) >= 8 and sent_groups == [cyc[(first + i) % 4] for i in range(len(sent_groups))]
            assert abs(int(res["groups_repeated"]) - len(sent_groups)) <= 1 and int(res["groups_no_room"]) == 0
        assert same(got, want), explain(got, want)
