"""What of dabgpu_packet_slides_dev and dabgpu_packet_fec_dev only device code can get wrong (csrc/packet_kernels.hip,
csrc/packet_fec_kernels.hip, csrc/wave_copy.hpp): how a frame is staged into LDS at its 16-byte phase, how frames map to lanes
and blocks, the packed scan record, the copy classes of the whole-wave copy, the ballot of the accept kernel, the lanes of the
Chien search, the split of an FEC frame between d_out and the new state record, the tally across lanes, the stage area.

The yardsticks are tests/packet_reference.py and tests/packet_fec_reference.py, run once per stream content; the host twins
(dabgpu_packet_slides_host, dabgpu_packet_fec_host) are held to them on the CPU for every new stream and stand in for the same
content at other phases, strides and cuts.  Every device result must equal the host twin's byte for byte: output, state
record, arena, result record, and every sentinel byte around them.  The CPU tests of part 1 say what the directed sets reach
(a census against closed forms of the contract's parameter ranges); the GPU tests run them.  See
tests/README_packet_device_edges.md."""
import copy
import os
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import packet_fec_reference as F
import test_packet as T
import test_packet_fec as E
import test_pad_slides as PS
from conftest import ROOT
from test_packet import pctx                                          # noqa: F401 (fixture)
from test_pad_device_edges import MOVE, SLIDE, census, classify, table
from test_wave_copy import SANITIZE

ADDR, FILL, GAP = T.ADDR, T.FILL, T.GAP
PACKET = 5                                                            # dabgpu_packet::ORDER_PACKET

_CACHE = {}


def cached(key, make):
    """streams and the references' answers: made once, shared, left as they are"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def slides_want(key, sp):
    return cached(("want",) + key, lambda: T.ref_call(T.receiver(sp), sp))


def equal_to_host(g, h):
    return g["state"].tobytes() == h["state"].tobytes() and (g["arena"] == h["arena"]).all() and g["result"].tobytes() == h["result"].tobytes()


# ================================================================================================ part 1: streams and census
# ---- scan staging: S = 1 .. 64, in_stride = 24 S + 1: a frame at every 16-byte phase
def staging_classes(S, a):
    """a frame of 24 S bytes at phase a of its room in LDS, as packet_scan_kernel stages it -> (ragged head bytes, full
    16-byte words, ragged tail bytes)"""
    n = 24 * S
    head = min(-a % 16, n)
    words = (n - head) // 16
    return head, words, n - head - 16 * words


def staging_stream(S):
    """a short object in packets of 1 .. 4 slots, one to a frame at a position that moves, a packet of another address
    behind it and padding packets around: every byte of every frame is under some packet's CRC"""
    def make():
        o = T.obj(0x700 + S, 700, 200 + S, b"stage %d" % S, 100)
        pk = T.exact_packets(o[2], ADDR, [L for L in (1, 2, 1, 3, 1, 4) if L <= S])
        other = synth.packet(9, b"beside", 1)
        rows = []
        for k, p in enumerate(pk):
            L = len(p) // 24
            pos = (5 * k) % (S - L + 1)
            rows.append([T.PAD1] * pos + [p] + ([other] if pos + L < S else []))
        rows += [[]] * (STAGING_FRAMES - len(rows))
        assert 17 <= len(pk) <= STAGING_FRAMES == len(rows), (S, len(pk))
        return dict(bitrate=8 * S, frames=T.frames_of(S, rows), slides=T.sent((0x700 + S, o)), body_capacity=1024, slide_stride=1024, followed=len(pk))
    return cached(("staging", S), make)


STAGING_FRAMES = 48


def staging_specs():
    return [T.spec_of(staging_stream(S), stride=24 * S + 1, in_off=(5 * S) % 16) for S in range(1, 65)]


def test_census_of_scan_staging():
    """Admitted: every (S, a), S = 1 .. 64 slots, a = 0 .. 15 the frame's address mod 16 (d_in may lie on any byte, in_stride is
    any number >= 24 S): 1024 pairs.  S and a fix the ragged head (-a mod 16 bytes), the full 16-byte words and the ragged tail.
    The 64 directed entries -- in_stride = 24 S + 1, odd mod 16, 48 frames -- reach all 1024, among them the frames without a
    full word (S = 1, a = 1 .. 7: 24 bytes that are head and tail only) and with one."""
    specs = staging_specs()
    reached = {(sp["bitrate"] // 8, (sp["in_off"] + k * sp["stride"]) % 16) for sp in specs for k in range(STAGING_FRAMES)}
    admitted = {(S, a) for S in range(1, 65) for a in range(16)}
    assert reached == admitted, sorted(admitted - reached)
    by_words = {}
    for S, a in sorted(reached):
        head, words, tail = staging_classes(S, a)
        assert head + 16 * words + tail == 24 * S and head < 16 and tail < 16
        by_words.setdefault(words, []).append((S, a, head, tail))
    print("full words of a staged frame: pairs (S, a)\n" + "\n".join("  %2d: %d" % (w, len(v)) for w, v in sorted(by_words.items())))
    assert sorted((S, a) for S, a, _h, _t in by_words[0]) == [(1, a) for a in range(1, 8)] and all(h + t == 24 for _S, _a, h, t in by_words[0])
    assert {(S, a) for S, a, _h, _t in by_words[1]} == {(1, a) for a in (0, 8, 9, 10, 11, 12, 13, 14, 15)}
    assert set(by_words) == set(range(0, 97)), sorted(by_words)
    # with S odd 24 S = 8 (mod 16): head and tail differ by 8; with S even they add up to 0 or 16
    for S, a in reached:
        head, _w, tail = staging_classes(S, a)
        assert (head + tail) % 16 == (8 if S % 2 else 0), (S, a)


@pytest.mark.parametrize("S", range(1, 65))
def test_staging_streams_host_equals_the_reference(built, S):
    st = staging_stream(S)
    sp = T.spec_of(st)
    want = slides_want(("staging", S), sp)
    got = T.call(T.HostMemory(), [sp], STAGING_FRAMES)[0]
    assert T.same(got, want), T.explain(got, want)
    assert [(int(r["transport_id"][0]), h, b) for r, h, b in want[0]] == st["slides"]
    assert int(want[1]["packets_followed"][0]) == st["followed"] and int(want[1]["slots_bad"][0]) == 0 and int(want[1]["continuity_breaks"][0]) == 0


def test_every_byte_of_a_staging_frame_shows_in_the_result(built):
    """S = 1 and 2: any one byte of any frame changed changes the counters (its packet's CRC fails): a frame staged wrongly in
    any byte cannot give the reference's result"""
    for S in (1, 2):
        sp = T.spec_of(staging_stream(S))
        want = slides_want(("staging", S), sp)[1].tobytes()
        for k in range(STAGING_FRAMES):
            for b in range(24 * S):
                fr = sp["frames"].copy()
                fr[k, b] ^= 1 << ((k + b) % 8)
                assert T.call(T.HostMemory(), [dict(sp, frames=fr)], STAGING_FRAMES)[0]["result"].tobytes() != want, (S, k, b)


# ---- row counts: the edges of the walk's `k += 64` record sum and `k0 += 64` ballot
ROW_COUNTS = (63, 64, 65, 128, 129)
ROW_SLOTS = (1, 3, 64)


def rows_stream(S, n):
    """n frames of padding but for: one followed packet (a data group of its own) in the first and last frame of every 64,
    and an object in the last frames, one packet to a frame, that closes in frame n - 1"""
    def make():
        o = T.obj(0x800 + S, 5, 300 + S, b"r", 64)
        last = synth.packetise(o[2], ADDR, sizes=(min(S, 4),))
        marked = sorted({k for k in range(n) if k % 64 in (0, 63)} | set(range(n - len(last), n)))
        pk = [T.one(synth.msc_data_group(6, b"m%d" % k)) for k in marked[:-len(last)]] + last
        assert len(pk) == len(marked) and len(last) < 60
        rows = [[] for _ in range(n)]
        for k, p in zip(marked, T.renumber(pk)):
            rows[k] = [T.PAD1] * (k % (S - len(p) // 24 + 1)) + [p]
        return dict(bitrate=8 * S, frames=T.frames_of(S, rows), slides=T.sent((0x800 + S, o)), body_capacity=64, followed=len(pk))
    return cached(("rows", S, n), make)


def rows_spec(S, n):
    return T.spec_of(rows_stream(S, n), stride=24 * S + (S % 3), in_off=S % 5)


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_count_streams_host_equals_the_reference(built, n):
    for S in ROW_SLOTS:
        st, sp = rows_stream(S, n), rows_spec(S, n)
        want = slides_want(("rows", S, n), sp)
        got = T.call(T.HostMemory(), [sp], n)[0]
        assert T.same(got, want), T.explain(got, want)
        assert [(int(r["transport_id"][0]), h, b) for r, h, b in want[0]] == st["slides"] and int(want[0][0][0]["superframe"][0]) == n - 1
        assert int(want[1]["packets_followed"][0]) == st["followed"] and int(want[1]["continuity_breaks"][0]) == 0
        assert int(want[1]["cifs"][0]) == n and int(want[1]["mot"]["groups_ignored_type"][0]) >= 1


# ---- full scan records at S = 64
def full_stream():
    def make():
        rng = np.random.default_rng(71)
        o = T.obj(0x900, 1300, 72, b"full.jpg", 200)
        pk = synth.packetise(o[2], ADDR, sizes=(1,))
        assert 64 < len(pk) <= 128 and all(len(p) == 24 for p in pk)
        bad = rng.integers(0, 256, (64, 24), dtype=np.uint8)
        bad[:, 0] |= 0xC0                                             # four slots long: overruns the frame or fails its CRC
        rows = [pk[:64], [T.PAD1] * 64, [synth.packet(5, b"other", 1)] * 64, [bytes(b) for b in bad], [synth.fec_packet(rng) for _ in range(64)], pk[64:]]
        return dict(bitrate=512, frames=T.frames_of(64, rows), slides=T.sent((0x900, o)), body_capacity=2048, slide_stride=2048, followed=len(pk))
    return cached("full", make)


def full_specs():
    st = full_stream()
    return [T.spec_of(st, fec=fec, stride=1536 + 3, in_off=7) for fec in (0, 1)]


def test_full_record_stream_host_equals_the_reference(built):
    """one frame each of 64 followed one-slot packets, 64 padding packets, 64 packets of another address, 64 bad slots and 64
    FEC-shaped slots (bad slots unless the entry's fec is set): the counts on the reference first"""
    st = full_stream()
    for fec, sp in zip((0, 1), full_specs()):
        want = slides_want(("full", fec), sp)
        got = T.call(T.HostMemory(), [sp], 6)[0]
        assert T.same(got, want), T.explain(got, want)
        counts = {k: int(want[1][k][0]) for k in ("slots_bad", "packets_fec", "packets_padding", "packets_other", "packets_followed")}
        assert counts == dict(slots_bad=64 + 64 * (1 - fec), packets_fec=64 * fec, packets_padding=64 + 128 - st["followed"], packets_other=64,
                              packets_followed=st["followed"]), counts
        assert [(int(r["transport_id"][0]), h, b) for r, h, b in want[0]] == st["slides"]


# ---- the walk's copy orders
def group_kw(src):
    """what puts a segment `src` bytes into its data group: 9 bytes of headers, an end-user address, an extension field"""
    assert 9 <= src <= 24
    return dict(end_user=bytes(src - 9)) if src <= 22 else dict(end_user=bytes(src - 11), extension=0xBEEF)


def placed(tid, size, last, src0, src1, seed):
    """an object whose body is one segment of `size` bytes and a last one of `last`; they lie src0 and src1 bytes into the
    group buffer and go to body offsets 0 and `size`"""
    body = T.image(size + last, seed)
    header = synth.slide_header(len(body), b"placed %x" % tid)
    groups = [synth.mot_group(3, tid, 0, True, header), synth.mot_group(4, tid, 0, False, body[:size], **group_kw(src0)),
              synth.mot_group(4, tid, 1, True, body[size:], continuity=1, **group_kw(src1))]
    return header, body, groups


def orders_stream():
    """The directed copies of the walk.  ORDER_MOVE: source 9 .. 24 bytes into the group buffer (arena offset 0), destination
    HEADER_OFF or BODY_OFF + n x segment size, both offsets multiples of 16: the second segment of an object with segments of
    48 + r bytes lands at phase r; it is moved by 16-byte words when it lies at phase r in its group, with a head of -r mod 16.
    ORDER_SLIDE: the header to byte 32 of its slot, the body behind it, at the header's length mod 16.  ORDER_PACKET: useful
    data lengths 1, 64, 65, 0 (no order) and 91 in one group."""
    def make():
        objs = []
        for r in range(16):                                           # 16-byte words, head -r mod 16
            objs.append(placed(0xA00 + r, 48 + r, 17 + (7 * r) % 30, 9 + r % 14, r if r >= 9 else 16 + r, 400 + r))
        for i, (q, size, last) in enumerate(((0, 64, 60), (1, 65, 2), (2, 66, 33), (3, 275, 260), (1, 69, 30))):
            objs.append(placed(0xA10 + i, size, last, 16, 12 if q == 0 else 8 + q, 420 + i))   # 4-byte words, head -q mod 4; shorter than its head (2 < 3)
        objs.append(placed(0xA15, 82, 70, 10, 9, 425))
        objs.append(placed(0xA16, 49, 13, 16, 17, 426))               # 16-byte words, shorter than its head (13 < 15)                # a byte a lane, more than one trip
        for i, (hb, bb) in enumerate(((32, 1009), (48, 1024), (20, 3), (24, 257), (28, 64), (17, 70), (18, 70))):
            objs.append(PS.sized_object(0xA20 + i, hb, bb, 430 + i))  # the body into its slot by 16-byte words, 4-byte words, bytes
        pk = synth.packetise(sum((o[2] for o in objs), []), ADDR, sizes=(4, 1, 3, 2))
        o = T.obj(0xA30, 250, 440, b"lengths", 2048)
        g = o[2][1]
        assert len(o[2]) == 2 and len(g) > 221
        pk += synth.packetise(o[2][:1], ADDR, sizes=(2,))
        pk += [T.one(g[0:1], last=False, slots=1), T.one(g[1:65], first=False, last=False, slots=3), T.one(g[65:130], first=False, last=False, slots=3),
               T.one(b"", first=False, last=False, slots=1), T.one(g[130:221], first=False, last=False, slots=4), T.one(g[221:], first=False)]
        objs.append(o)
        tids = list(range(0xA00, 0xA10)) + list(range(0xA10, 0xA17)) + list(range(0xA20, 0xA27)) + [0xA30]
        slides = [(tid, x[0], x[1]) for tid, x in zip(tids, objs)]
        return dict(bitrate=64, frames=synth.packet_frames(64, [T.renumber(pk)]), slides=slides, body_capacity=2048, slide_stride=2048, max_slides=len(objs))
    return cached("orders", make)


def test_orders_stream_host_equals_the_reference(built):
    st = orders_stream()
    sp = T.spec_of(st)
    want = slides_want(("orders",), sp)
    got = T.call(T.HostMemory(), [sp], len(sp["frames"]))[0]
    assert T.same(got, want), T.explain(got, want)
    assert [(int(r["transport_id"][0]), h, b) for r, h, b in want[0]] == st["slides"]
    assert int(want[1]["continuity_breaks"][0]) == 0 and int(want[1]["slots_bad"][0]) == 0 and int(want[1]["mot"]["slides_dropped"][0]) == 0


def run_order_census(tmp_path, sp):
    """tests/packet_order_census.cpp under AddressSanitizer and UBSan on one stream -> (orders [(kind, src, dst, len)],
    followed packets [(frame, pos, slots, udl, orders)], the bytes the orders left)"""
    exe, path = str(tmp_path / "packet_order_census"), str(tmp_path / "orders.stream")
    subprocess.check_call([a for a in SANITIZE if not a.startswith("-I")] + ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "packet_order_census.cpp"), "-o", exe])
    S = sp["bitrate"] // 8
    with open(path, "wb") as f:
        f.write(np.array([S, sp.get("address", ADDR), sp.get("fec", 0), sp["body_capacity"], sp.get("max_slides", 4), T.stride_of(sp), len(sp["frames"])], np.int32).tobytes())
        f.write(np.ascontiguousarray(sp["frames"]).tobytes())
    r = subprocess.run([exe, path, path + ".out"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-600:] + r.stderr[-2000:])
    orders = [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines() if l[:1].isdigit()]
    packets = [tuple(int(x) for x in l.split()[1:]) for l in r.stdout.splitlines() if l[:2] == "P "]
    return orders, packets, open(path + ".out", "rb").read()


def test_census_of_walk_copy_orders(built, tmp_path):
    """Every order of the directed stream, from the stand-alone census program (clean under ASan and UBSan; it refuses an
    ORDER_MOVE that overlaps its source and any order out of bounds, and holds walk_frames() to the orders it printed),
    classified as wave_copy() takes it.  Admitted, from the arena's layout (group buffer at 0, HEADER_OFF and BODY_OFF
    multiples of 16, slots and slot stride on 16 bytes):
      ORDER_MOVE   16-byte words with every head 0 .. 15, 4-byte words with every head 0 .. 3, bytes; tails zero and not; a
                   copy shorter than its head on either word class
      ORDER_SLIDE  all three classes, tails zero and not -- and no head, ever: its source is HEADER_OFF or BODY_OFF, so where
                   source and destination share a phase the destination is aligned (asserted: should the layout change, the
                   census will ask for the heads)
      ORDER_PACKET lengths 1, 64, 65 and 91 (the byte loop: one lane, a full trip, a second trip, the longest there is).  A
                   length of 0 cannot occur: Sink::order() leaves no order for no bytes.  The packet without useful bytes is
                   in the stream and is followed: it leaves no order at all (asserted).
    As printed by this test:
      MOVE   1-byte  copies  54  longer than one trip of the wave (64 bytes): 8 | source and destination two bytes apart (mod 4): 6
      MOVE   4-byte  copies   7  heads 0:3 1:1 3:1  other:2 | words 0:1 1:0 63:0 64:1 65:0  other:5 | tails 0:2 1:0 3:5  other:0 | len < head: 1
      MOVE  16-byte  copies  24  heads 0:8 1:1 7:1 15:1  other:13 | words 0:5 1:9 63:0 64:0 65:0  other:10 | tails 0:2 1:5 15:2  other:15 | len < head: 1
      SLIDE  1-byte  copies  26  longer than one trip of the wave (64 bytes): 25 | source and destination two bytes apart (mod 4): 2
      SLIDE  4-byte  copies   3  heads 0:3 1:0 3:0  other:0 | words 0:1 1:0 63:0 64:1 65:0  other:1 | tails 0:1 1:1 3:1  other:0 | len < head: 0
      SLIDE 16-byte  copies  33  heads 0:33 1:0 7:0 15:0  other:0 | words 0:0 1:29 63:1 64:1 65:0  other:2 | tails 0:3 1:2 15:0  other:28 | len < head: 0
    (the trips of the word loop -- 63, 64 and 65 words -- are the PAD streams' and tests/wave_copy_exhaustive.cpp's: the copy
    is the same header.)
    """
    st = orders_stream()
    sp = T.spec_of(st)
    orders, packets, left = run_order_census(tmp_path, sp)
    cs = census(orders)
    print(table(cs))
    for kind in (MOVE, SLIDE):
        assert {B for k, B in cs if k == kind} == {1, 4, 16}, kind
        for B in (4, 16):
            c = cs[(kind, B)]
            assert c["tails"].get(0) and set(c["tails"]) - {0}, (kind, B, c)
            if kind == MOVE:
                assert set(c["heads"]) == set(range(B)) and c["short"] >= 1, (B, c)
            else:
                assert set(c["heads"]) == {0} and c["short"] == 0, (B, c)
        assert cs[(kind, 1)]["heads"].get(2) and set(cs[(kind, 1)]["heads"]) & {1, 3}, (kind, cs[(kind, 1)])
        assert any(n > 64 for k, s_, d_, n in orders if k == kind and classify(s_, d_, n)[0] == 1), kind
    lengths = {n for k, _s, _d, n in orders if k == PACKET}
    assert lengths >= {1, 64, 65, 91} and 0 not in lengths and max(lengths) == 91, sorted(lengths)
    assert any(udl == 0 and n == 0 for _k, _pos, _L, udl, n in packets) and all(n >= 1 for _k, _pos, _L, udl, n in packets if udl)
    # what the orders left is what the host twin leaves: arena, state record, counters
    got = T.call(T.HostMemory(), [sp], len(sp["frames"]))[0]
    ab, nb = dabgpu.mot_arena_bytes(sp["body_capacity"]), dabgpu.packet_state_bytes()
    slots = sp["max_slides"] * T.stride_of(sp)
    assert len(left) == ab + slots + nb + 192
    assert left[:ab] == got["arena"].tobytes() and left[ab + slots:ab + slots + nb] == got["state"].tobytes() and left[ab + slots + nb:] == got["result"].tobytes()


# ---- the FEC move kernel's copies: a closed form of the entry
#: (bit rate, d_in mod 16, in_stride - 24 S, out_stride - 24 S, how far output frame k + D lies from input frame k, mod 16, where
#: the two strides are equal: d_out mod 16 follows from it)
MOVE_ENTRIES = [(8, 9, 1, 1, 0),      # S = 1: equal drift, equal phase: 16-byte words at every head, 9 .. 15 without a word
                (8, 0, 1, 1, 4),      # ... 4 apart: 4-byte words at every head
                (8, 0, 1, 2, 0),      # ... unequal drift: bytes
                (8, 8, 0, 0, 0),      # ... frames on phases 8, 0, 8, ... into the record's 0, 8, 0, ...
                (16, 5, 1, 1, 0), (24, 0, 0, 0, 0), (24, 7, 3, 3, 8), (40, 2, 5, 5, 4), (128, 1, 0, 0, 8), (264, 4, 9, 9, 0), (512, 11, 7, 7, 0), (512, 0, 16, 0, 3)]
#: (first frame, n_cifs, the call whose state it continues): 120 frames from a fresh start, then 34 and, again from the first
#: call's state, 21: above every D; below, equal to and above
MOVE_CALLS = [(0, 120, None), (120, 34, 0), (120, 21, 0)]
MOVE_FRAMES = 154


def move_copies(S, n, carried, d_in, in_stride, d_out, out_stride):
    """the wave_copy() calls of packet_fec_move_kernel for one entry (state records on 16 bytes: the ABI) -> [(kind, src, dst,
    len)], addresses mod 16 where it matters"""
    D, fb, out = F.delay(8 * S), 24 * S, []
    for wf in range(D + n):
        to_out = wf < n
        dst = d_out + wf * out_stride if to_out else 64 + (wf - n) * fb
        if wf >= D:
            out.append(("frame to " + ("d_out" if to_out else "state"), d_in + (wf - D) * in_stride, dst, fb))
        elif carried:
            out.append(("carried to " + ("d_out" if to_out else "state"), 64 + wf * fb, dst, fb))
    return out


ANY = {(16, h) for h in range(16)} | {(4, h) for h in range(4)} | {(1, None)}
HALF = {(16, 0), (16, 8), (4, 0)}
#: the record's frames lie on phase 0 or 8 (64 + k 24 S), frames of the caller's on any: which (bytes per access, head) can be
MOVE_ADMITTED = {"frame to d_out": ANY, "frame to state": HALF | {(1, None)}, "carried to d_out": HALF | {(1, None)}, "carried to state": HALF}


def move_specs():
    return [dict(bitrate=br, stride=3 * br + ds, out_stride=3 * br + do, in_off=a, out_off=(a + delta - F.delay(br) * (3 * br + do)) % 16) for br, a, ds, do, delta in MOVE_ENTRIES]


def test_census_of_fec_move_copies():
    """Admitted per kind of copy, from the ranges of the contract (d_in, d_out on any byte, strides any number >= 24 S, state
    records on 16 bytes, their frames at 64 + k 24 S: phase 0, or 8 where S and k are odd): see MOVE_ADMITTED.  A frame between
    two state records is never moved by bytes (both phases are 0 or 8).  The directed entries, over the three calls, reach
    every admitted class; S = 1 reaches heads 9 .. 15 on 16-byte words, copies of 24 bytes without one full word; odd S writes
    the record's frames at phase 0 and 8 by turns."""
    reached, wordless, phases = {}, set(), set()
    for sp in move_specs():
        S = sp["bitrate"] // 8
        for first, n, state in MOVE_CALLS:
            for kind, src, dst, fb in move_copies(S, n, state is not None, sp["in_off"] + first * sp["stride"], sp["stride"], sp["out_off"], sp["out_stride"]):
                B, head, words, _tail, short = classify(src, dst, fb)
                reached.setdefault(kind, set()).add((B, head if B > 1 else None))
                assert not short
                if S == 1 and B == 16 and words == 0:
                    wordless.add(head)
                if S % 2 and kind.endswith("state"):
                    phases.add((S, dst % 16))
    for kind, cl in sorted(reached.items()):
        print("%-17s %s" % (kind, " ".join("%d/%s" % c for c in sorted(cl, key=lambda c: (c[0], c[1] or 0)))))
    assert reached == MOVE_ADMITTED, {k: sorted(MOVE_ADMITTED[k] ^ reached.get(k, set()), key=str) for k in MOVE_ADMITTED}
    assert wordless == set(range(9, 16)), wordless
    assert phases >= {(S, p) for S in (1, 3, 5, 33) for p in (0, 8)}, phases
    D = {sp["bitrate"]: F.delay(sp["bitrate"]) for sp in move_specs()}
    for _first, n, _state in MOVE_CALLS[1:]:
        assert any(n < d for d in D.values()) and any(n > d for d in D.values())
    assert 34 in D.values() and 21 in D.values() and all(MOVE_CALLS[0][1] > d for d in D.values())


def move_stream(bitrate):
    """154 frames: three FEC frames with a wiped packet each, padding behind them"""
    def make():
        fr = E.clean_frames(bitrate, 500 + bitrate)
        if len(fr) < MOVE_FRAMES:
            fr = np.concatenate([fr, synth.packet_frames(bitrate, [], n_frames=MOVE_FRAMES - len(fr))])
        fr = fr[:MOVE_FRAMES].copy()
        rng = np.random.default_rng(bitrate)
        for t in range(3):
            if (103 * t + 103) * 24 <= fr.size:
                E.wipe(fr, 103 * t + 13 + 31 * t, rng)
        return fr
    return cached(("move", bitrate), make)


def move_wants(bitrate):
    """the reference's answers to the three calls"""
    def make():
        fr = move_stream(bitrate)
        rx = F.Receiver(bitrate)
        first = rx.call(fr[:120])
        other = copy.deepcopy(rx)
        return [first, rx.call(fr[120:154]), other.call(fr[120:141])]
    return cached(("move want", bitrate), make)


@pytest.mark.parametrize("bitrate", sorted({e[0] for e in MOVE_ENTRIES}))
def test_move_streams_host_equals_the_reference(built, bitrate):
    fr, wants = move_stream(bitrate), move_wants(bitrate)
    first = E.call(E.HostMemory(), [dict(bitrate=bitrate, frames=fr)], 120)[0]
    assert (first["out"] == wants[0][0]).all() and first["result"].tobytes() == wants[0][1].tobytes()
    assert E.counts_of(wants[0][1])["rows_corrected"] >= 12
    for (a, n, _s), want in zip(MOVE_CALLS[1:], wants[1:]):
        got = E.call(E.HostMemory(), [dict(bitrate=bitrate, frames=fr[a:a + n], state=first["state"].tobytes())], n)[0]
        assert (got["out"] == want[0]).all() and got["result"].tobytes() == want[1].tobytes(), (bitrate, n)


# ---- accept edges: where in the ballot of 64 new slots a frame ends
BASE_TABLES = 5


def base_slots():
    """five clean FEC frames, slot by slot: what the accept and split streams are cut from"""
    return cached("base", lambda: E.clean_frames(512, 600, tables=BASE_TABLES).reshape(-1, 24)[:103 * BASE_TABLES].copy())


def ending_at(S, e, n_frames, wiped=20, seed=0):
    """n_frames logical frames of S slots cut from the base so that an FEC frame ends at slot e of them (e >= 102: it is whole),
    slot `wiped` of that FEC frame overwritten (None: as sent)"""
    t = e // 103
    s0 = 103 * t + 102 - e
    slots = base_slots()[s0:s0 + n_frames * S].copy()
    assert len(slots) == n_frames * S and e >= 102 and F.mark(slots[e]) == 8
    if wiped is not None:
        E.wipe(slots, e - 102 + wiped, np.random.default_rng(1000 * S + e + seed))
    return slots.reshape(n_frames, 24 * S)


ACCEPT_J = tuple(range(9)) + (63, 64, 65)
#: S: (frames of the first call, of the second)
ACCEPT_CALLS = {4: (30, 20), 64: (2, 2)}
OVERLAP_J = 40


def accept_streams(S):
    """per new-slot j of the second call at which the FEC frame ends: the frames of both calls; and, last, the stream whose
    nine marks are there again, ending 10 slots before the real end (j = 30 and 40: one ballot)"""
    def make():
        n1, n2 = ACCEPT_CALLS[S]
        out = [ending_at(S, n1 * S + j, n1 + n2) for j in ACCEPT_J]
        fr = ending_at(S, n1 * S + OVERLAP_J, n1 + n2)
        flat, e = fr.reshape(-1, 24), n1 * S + OVERLAP_J
        for i in range(9):
            flat[e - 18 + i] = flat[e - 8 + i]
        return out + [fr]
    return cached(("accept", S), make)


def accept_wants(S):
    def make():
        n1 = ACCEPT_CALLS[S][0]
        out = []
        for fr in accept_streams(S):
            rx = F.Receiver(8 * S)
            out.append((rx.call(fr[:n1]), rx.call(fr[n1:])))
        return out
    return cached(("accept want", S), make)


@pytest.mark.parametrize("S", sorted(ACCEPT_CALLS))
def test_accept_streams_host_equals_the_reference(built, S):
    """on the reference first: the frame ends in the second call, whole, and is corrected; in the last stream the repeated
    marks are taken for a frame's end and the real end, 10 slots on, overlaps it"""
    n1, n2 = ACCEPT_CALLS[S]
    streams, wants = accept_streams(S), accept_wants(S)
    specs = [dict(bitrate=8 * S, frames=fr[:n1]) for fr in streams]
    first = E.call(E.HostMemory(), specs, n1)
    second = E.call(E.HostMemory(), [dict(bitrate=8 * S, frames=fr[n1:], state=f["state"].tobytes()) for fr, f in zip(streams, first)], n2)
    for k, (f, s, (w1, w2)) in enumerate(zip(first, second, wants)):
        assert (f["out"] == w1[0]).all() and f["result"].tobytes() == w1[1].tobytes(), (S, k)
        assert (s["out"] == w2[0]).all() and s["result"].tobytes() == w2[1].tobytes(), (S, k)
        c = E.counts_of(w2[1])
        if k < len(ACCEPT_J):
            assert c["frames"] in (1, 2) and (c["frames_overlapping"], c["rows_corrected"], c["rows_uncorrectable"]) == (0, 12, 0), (S, k, c)   # (at S = 64 the next frame ends in the call, too)
        else:
            assert (c["frames"], c["frames_overlapping"]) == (1, 1), (S, c)


# ---- Chien search: every position, every lane
def chien_streams():
    """`positions`: 17 FEC frames at 512 kbit/s whose 204 rows carry one error each, at codeword positions 0 .. 203 in turn
    (row r of frame t: position 12 t + r).  `lanes`: two FEC frames at 256 kbit/s; in the first, row r carries eight errors at
    positions = r (mod 16), all found by one of the row's 16 lanes; in the second, eight errors on eight different residues,
    found by eight lanes at once."""
    def make():
        rng = np.random.default_rng(77)
        pos = E.clean_frames(512, 601, tables=17)
        sent = pos.copy()
        for t in range(17):
            for r in range(12):
                E.hit(pos, t, r, [12 * t + r], rng=rng)
        lanes = E.clean_frames(256, 602, tables=2)
        for r in range(12):
            E.hit(lanes, 0, r, rng.choice(np.arange(r, 204, 16), 8, replace=False), rng=rng)
            E.hit(lanes, 1, r, [int(q) + 16 * int(rng.integers(0, (203 - q) // 16 + 1)) for q in rng.choice(16, 8, replace=False)], rng=rng)
        return dict(positions=dict(bitrate=512, frames=pos, sent=sent), lanes=dict(bitrate=256, frames=lanes))
    return cached("chien", make)


def fec_want(key, st):
    return cached(("fec want", key), lambda: F.Receiver(st["bitrate"]).call(st["frames"]))


def test_chien_streams_host_equals_the_reference(built):
    sts = chien_streams()
    for name, st in sts.items():
        want = fec_want(name, st)
        got = E.call(E.HostMemory(), [dict(bitrate=st["bitrate"], frames=st["frames"])], len(st["frames"]))[0]
        assert (got["out"] == want[0]).all() and got["result"].tobytes() == want[1].tobytes(), name
    c = E.counts_of(fec_want("positions", sts["positions"])[1])
    assert (c["frames"], c["rows_corrected"], c["rows_clean"], c["bytes_corrected"], c["parity_bytes_corrected"]) == (17, 204, 0, 188, 16), c
    pos = sts["positions"]
    data = np.arange(17 * 103) % 103 < 94
    assert (fec_want("positions", pos)[0][2:].reshape(-1, 24)[:17 * 103][data] == pos["sent"][:-2].reshape(-1, 24)[:17 * 103][data]).all(), "the data as sent"
    c = E.counts_of(fec_want("lanes", sts["lanes"])[1])
    assert (c["frames"], c["rows_corrected"], c["bytes_corrected"] + c["parity_bytes_corrected"]) == (2, 24, 192) and c["parity_bytes_corrected"] > 0, c


# ---- the split of an FEC frame between d_out and the new state record
SPLIT_SLOTS = (2, 3, 5, 7, 16, 33, 63, 64)


def split_streams(S):
    """Three calls of D frames each.  The FEC frame that ends in the second call at new slot j = 102 - p has its first p slots
    in that call's d_out and its other 103 - p in the new state record (window slot D S + j - 102 + p = D S: the first of
    the record).  p = 1 .. 102 are all there are (p = 0 or 103: no split).  One entry per p; the wiped packet is the last slot
    in d_out (p odd) or the first in the record (p even), among the 94 data slots.  The third call's frames are padding: it
    brings out what the record held."""
    def make():
        D = F.delay(8 * S)
        out = []
        for p in range(1, 103):
            fr = ending_at(S, D * S + 102 - p, 2 * D, wiped=min(p - 1 if p % 2 else p, 93))
            out.append(np.concatenate([fr, synth.packet_frames(8 * S, [], n_frames=D)]))
        return out
    return cached(("split", S), make)


def split_wants(S):
    def make():
        D = F.delay(8 * S)
        out = []
        for fr in split_streams(S):
            rx = F.Receiver(8 * S)
            out.append([rx.call(fr[k * D:(k + 1) * D]) for k in range(3)])
        return out
    return cached(("split want", S), make)


@pytest.mark.parametrize("S", SPLIT_SLOTS)
def test_split_streams_host_equals_the_reference(built, S):
    D = F.delay(8 * S)
    streams, wants = split_streams(S), split_wants(S)
    state = [None] * len(streams)
    for k in range(3):
        got = E.call(E.HostMemory(), [dict(bitrate=8 * S, frames=fr[k * D:(k + 1) * D], state=s) for fr, s in zip(streams, state)], D)
        for p, (g, w) in enumerate(zip(got, wants), 1):
            assert (g["out"] == w[k][0]).all() and g["result"].tobytes() == w[k][1].tobytes(), (S, p, k)
        state = [g["state"].tobytes() for g in got]
    for p, (fr, w) in enumerate(zip(streams, wants), 1):              # on the reference: the frame ends in the second call and comes out as sent
        c = E.counts_of(w[1][1])
        # (a wiped packet is two random bytes in each row; in a few of these 816 streams one row's two are the bytes that were sent)
        assert c["frames"] >= 1 and c["rows_corrected"] >= 11 and c["rows_uncorrectable"] == 0, (S, p, c)
        e = D * S + 102 - p
        sent = ending_at(S, e, 2 * D, wiped=None).reshape(-1, 24)[e - 102:e - 8]
        out = np.concatenate([x[0] for x in w]).reshape(-1, 24)[D * S + e - 102:D * S + e - 8]
        assert (fr[:2 * D].reshape(-1, 24)[e - 102:e - 8] != sent).any() and (out == sent).all(), (S, p)


# ---- tally
def tally_streams():
    """66 FEC frames at 512 kbit/s (109 logical frames): frame k carries k mod 9 errors in row k mod 12, from the second on one
    of them in the parity, and every eleventh frame ten errors in another row, beyond the bound; and two FEC frames beside
    them in an entry of its own"""
    def make():
        rng = np.random.default_rng(88)
        fr = E.clean_frames(512, 603, tables=66)
        for k in range(66):
            n = k % 9
            if n:
                where = [188 + k % 16] if n > 1 else []
                where += [int(c) for c in rng.choice(188, n - len(where), replace=False)]
                E.hit(fr, k, k % 12, where, rng=rng)
            if k % 11 == 5:
                E.hit(fr, k, (k + 6) % 12, rng.choice(204, 10, replace=False), rng=rng)
        two = E.clean_frames(512, 604, tables=2)
        E.wipe(two, 50, rng)
        return dict(many=dict(bitrate=512, frames=fr), two=dict(bitrate=512, frames=two))
    return cached("tally", make)


def test_tally_streams_host_equals_the_reference(built):
    sts = tally_streams()
    for name, st in sts.items():
        want = fec_want("tally " + name, st)
        got = E.call(E.HostMemory(), [dict(bitrate=st["bitrate"], frames=st["frames"])], len(st["frames"]))[0]
        assert (got["out"] == want[0]).all() and got["result"].tobytes() == want[1].tobytes(), name
    c = E.counts_of(fec_want("tally many", sts["many"])[1])
    errors = sum(k % 9 for k in range(66))
    assert (c["frames"], c["rows_corrected"], c["rows_uncorrectable"]) == (66, 66 - 8, 6) and c["rows_clean"] == 66 * 12 - 58 - 6, c
    assert c["parity_bytes_corrected"] == sum(k % 9 > 1 for k in range(66)) and c["bytes_corrected"] + c["parity_bytes_corrected"] == errors, c
    assert len(sts["many"]["frames"]) == 109 and E.counts_of(fec_want("tally two", sts["two"])[1])["frames"] == 2


# ================================================================================================ several calls on one image
class Image:
    """One allocation for the buffers of several calls, every region between sentinel bytes, on a 256-byte boundary plus an
    offset of its own.  The same calls run on a copy in host memory (the host twins) and on a copy in device memory, back to
    back with nothing waiting in between: the two images must come out the same, byte for byte -- outputs, state records,
    arenas, results and every byte around them -- and the host's must have changed in its output regions only."""

    def __init__(self):
        self.size, self.data, self.outputs = 0, [], []

    def take(self, n, off=0, data=None, output=False):
        at = (self.size + GAP + 255) // 256 * 256 + off
        self.size = at + n
        if data is not None:
            self.data.append((at, np.frombuffer(bytes(data), np.uint8)))
        if output:
            self.outputs.append((at, n))
        return at

    def rows(self, frames, stride, off=0):
        """frames [n][bytes] at a row stride -> offset of the first"""
        n, fb = frames.shape
        at = self.take(max(n, 1) * stride + 16, off)
        for k in range(n):
            self.data.append((at + k * stride, frames[k]))
        return at

    def run(self, ctx, calls):
        """calls: [(kind "fec" / "slides", base -> entries, n_cifs)] -> the image after them"""
        import torch
        img = np.full(self.size + GAP, FILL, np.uint8)
        for at, d in self.data:
            img[at:at + len(d)] = d
        raw = np.empty(img.size + 256, np.uint8)
        off = -raw.ctypes.data % 256
        host = raw[off:off + img.size]
        host[:] = img
        for kind, entries, n in calls:
            (dabgpu.packet_fec_host if kind == "fec" else dabgpu.packet_slides_host)(entries(host.ctypes.data), n)
        may = np.zeros(img.size, bool)
        for at, n in self.outputs:
            may[at:at + n] = True
        assert (host[~may] == img[~may]).all(), "the host call wrote outside its outputs"
        dev = torch.from_numpy(img).cuda()
        assert dev.data_ptr() % 256 == 0
        for kind, entries, n in calls:                                # nothing waits between the calls
            (ctx.packet_fec_dev if kind == "fec" else ctx.packet_slides_dev)(entries(dev.data_ptr()), n)
        ctx.sync()
        got = dev.cpu().numpy()
        if not (got == host).all():
            bad = np.flatnonzero(got != host)
            where = [(at, n) for at, n in self.outputs if at <= bad[0] < at + n]
            raise AssertionError("device and host differ in %d bytes, the first at %d (output region %s): %s / %s" % (
                len(bad), bad[0], where or "none: a sentinel", got[bad[:8]], host[bad[:8]]))
        return host.copy()


class FecCall:
    """one dabgpu_packet_fec call on an Image: specs as test_packet_fec.call takes them, `frames_at` (offsets) where an earlier
    call has laid the frames down, `first` the row it begins at, `states` the offsets of the records it continues"""

    def __init__(self, im, specs, n, frames_at=None, first=0, states=None):
        self.n, self.lay = n, []
        for e, sp in enumerate(specs):
            fb, nb = 3 * sp["bitrate"], dabgpu.packet_fec_state_bytes(sp["bitrate"])
            stride, ostride = sp.get("stride", fb), sp.get("out_stride", fb)
            frames = frames_at[e] if frames_at else im.rows(sp["frames"], stride, sp.get("in_off", 0))
            L = dict(bitrate=sp["bitrate"], fb=fb, nb=nb, stride=stride, ostride=ostride, frames=frames, d_in=frames + first * stride,
                     out=im.take(max(n, 1) * ostride + 16, sp.get("out_off", 0)), sin=states[e] if states else None, sout=im.take(nb, output=True),
                     result=im.take(48, output=True))
            im.outputs += [(L["out"] + k * ostride, fb) for k in range(n)]
            self.lay.append(L)

    def entries(self, base):
        return [dabgpu.PacketFecEntry(base + L["d_in"], L["stride"], L["bitrate"], 0, base + L["out"], L["ostride"], base + L["sin"] if L["sin"] is not None else None,
                                      base + L["sout"], base + L["result"]) for L in self.lay]

    def call(self):
        return ("fec", self.entries, self.n)

    def read(self, img):
        return [dict(out=np.stack([img[L["out"] + k * L["ostride"]:L["out"] + k * L["ostride"] + L["fb"]] for k in range(self.n)]) if self.n else np.zeros((0, L["fb"]), np.uint8),
                     result=img[L["result"]:L["result"] + 48].copy().view(dabgpu.PACKET_FEC_RESULT_DTYPE), state=img[L["sout"]:L["sout"] + L["nb"]].copy()) for L in self.lay]


class SlidesCall:
    """one dabgpu_packet_slides call on an Image, from a fresh start: specs as test_packet.call takes them"""

    def __init__(self, im, specs, n):
        self.n, self.lay, self.specs = n, [], specs
        nb = dabgpu.packet_state_bytes()
        for sp in specs:
            stride, ab = sp.get("stride", 3 * sp["bitrate"]), dabgpu.mot_arena_bytes(sp["body_capacity"])
            slots = max(sp.get("max_slides", 4), 1) * T.stride_of(sp)
            self.lay.append(dict(stride=stride, ab=ab, frames=im.rows(sp["frames"][:n], stride, sp.get("in_off", 0)), sout=im.take(nb, output=True),
                                 arena=im.take(ab, output=True), slides=im.take(slots, output=True), result=im.take(192, output=True)))

    def entries(self, base):
        return [dabgpu.PacketEntry(base + L["frames"], L["stride"], sp["bitrate"], sp.get("address", ADDR), sp.get("fec", 0), 0, None, base + L["sout"], base + L["arena"],
                                   L["ab"], base + L["slides"], T.stride_of(sp), sp.get("max_slides", 4), 0, base + L["result"]) for sp, L in zip(self.specs, self.lay)]

    def call(self):
        return ("slides", self.entries, self.n)

    def read(self, img):
        """-> per entry what test_packet.call gives; the slots hold nothing but the slides the result counts"""
        out = []
        for sp, L in zip(self.specs, self.lay):
            res = img[L["result"]:L["result"] + 192].copy().view(dabgpu.PACKET_RESULT_DTYPE)
            slides, stride = [], T.stride_of(sp)
            region = img[L["slides"]:L["slides"] + max(sp.get("max_slides", 4), 1) * stride].copy()
            for k in range(int(res["mot"]["slides_written"][0])):
                rec = region[k * stride:k * stride + 32].copy().view(dabgpu.MOT_SLIDE_DTYPE)
                hb, bb = int(rec["header_bytes"][0]), int(rec["body_bytes"][0])
                assert 0 <= hb and 0 <= bb and 32 + hb + bb <= stride
                slides.append((rec, region[k * stride + 32:k * stride + 32 + hb].tobytes(), region[k * stride + 32 + hb:k * stride + 32 + hb + bb].tobytes()))
                region[k * stride:k * stride + 32 + hb + bb] = FILL
            assert (region == FILL).all(), "bytes of the slots outside the slides changed"
            out.append(dict(slides=slides, result=res, state=img[L["sout"]:L["sout"] + dabgpu.packet_state_bytes()].copy(), arena=img[L["arena"]:L["arena"] + L["ab"]].copy()))
        return out


# ============================================================================================================ part 2: GPU
def both(pctx, specs, n, **kw):
    """one slides call on device and on host memory (test_packet.call: every sentinel byte checked on either)"""
    return T.call(T.DeviceMemory(pctx), specs, n, **kw), T.call(T.HostMemory(), specs, n, **kw)


@pytest.mark.gpu
def test_gpu_scan_staging_every_slot_count_at_every_phase(pctx):
    """1. the 64 staging entries in ONE call: S = 1 .. 64, each frame of an entry at another 16-byte phase (in_stride = 24 S + 1):
    slides and counters equal the reference's (run per S), state and arena the host call's"""
    specs = staging_specs()
    got, host = both(pctx, specs, STAGING_FRAMES)
    for S, (sp, g, h) in enumerate(zip(specs, got, host), 1):
        want = slides_want(("staging", S), sp)
        assert T.same(g, want), "S = %d" % S + T.explain(g, want)
        assert T.same(h, want) and equal_to_host(g, h), S
        assert len(g["slides"]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_gpu_row_counts_around_the_wave(pctx, n):
    """2. n_cifs = 63, 64, 65, 128, 129 at S = 1, 3 and 64: followed packets in the first and last frame of every 64, a slide
    that closes in the last frame"""
    specs = [rows_spec(S, n) for S in ROW_SLOTS]
    got, host = both(pctx, specs, n)
    for S, sp, g, h in zip(ROW_SLOTS, specs, got, host):
        want = slides_want(("rows", S, n), sp)
        assert T.same(g, want), "S = %d" % S + T.explain(g, want)
        assert T.same(h, want) and equal_to_host(g, h), S
        assert len(g["slides"]) == 1 and int(g["slides"][0][0]["superframe"][0]) == n - 1


@pytest.mark.gpu
def test_gpu_full_scan_records(pctx):
    """3. S = 64: frames of 64 followed one-slot packets (a full list), 64 padding packets, 64 packets of another address, 64 bad
    slots, 64 FEC-shaped slots, read by an entry with fec = 0 and one with fec = 1 on the same d_in: the counters exact, and
    the slide that only comes out when all 64 followed packets were listed in order"""
    specs = full_specs()
    got, host = both(pctx, specs, 6, shared={1: 0})
    for fec, (sp, g, h) in enumerate(zip(specs, got, host)):
        want = slides_want(("full", fec), sp)
        assert T.same(g, want), "fec = %d" % fec + T.explain(g, want)
        assert T.same(h, want) and equal_to_host(g, h), fec
        assert len(g["slides"]) == 1 and int(g["result"]["packets_fec"][0]) == 64 * fec


@pytest.mark.gpu
def test_gpu_directed_copy_orders(pctx):
    """4. the directed stream of the census, at d_in on and off 16 bytes: every copy class of the walk kernel"""
    st = orders_stream()
    specs = [T.spec_of(st, in_off=off, stride=192 + extra) for off, extra in ((0, 0), (5, 0), (8, 7))]
    n = len(st["frames"])
    got, host = both(pctx, specs, n)
    want = slides_want(("orders",), specs[0])
    for sp, g, h in zip(specs, got, host):
        assert T.same(g, want), "in_off = %d" % sp["in_off"] + T.explain(g, want)
        assert T.same(h, want) and equal_to_host(g, h), sp["in_off"]
    assert len(got[0]["slides"]) == len(st["slides"])


@pytest.mark.gpu
def test_gpu_fec_move_copies(pctx):
    """5. the entries of the move census in one call of 120 frames from a fresh start, then two calls (34 and 21 frames) from
    the state record the first left on the device: frames and carried frames to d_out and to the new record, in every class
    of copy.  Device image equals host image; the outputs equal the reference's"""
    im = Image()
    specs = [dict(sp, frames=move_stream(sp["bitrate"])) for sp in move_specs()]
    first = FecCall(im, specs, 120)
    later = [FecCall(im, specs, n, frames_at=[L["frames"] for L in first.lay], first=a, states=[L["sout"] for L in first.lay]) for a, n, _s in MOVE_CALLS[1:]]
    img = im.run(pctx, [c.call() for c in [first] + later])
    for k, c in enumerate([first] + later):
        for sp, g in zip(specs, c.read(img)):
            want = move_wants(sp["bitrate"])[k]
            assert (g["out"] == want[0]).all() and g["result"].tobytes() == want[1].tobytes(), (k, sp["bitrate"], sp["in_off"])


@pytest.mark.gpu
@pytest.mark.parametrize("S", sorted(ACCEPT_CALLS))
def test_gpu_fec_accept_edges(pctx, S):
    """6. a second call, on the state of the first, in which the FEC frame ends at new slot 0, 1, .. 8 (its marks straddle the
    carried tail), 63, 64 and 65 (the ballot's edge); and two candidates in one ballot, the second overlapping the first"""
    n1, n2 = ACCEPT_CALLS[S]
    streams, wants = accept_streams(S), accept_wants(S)
    specs = [dict(bitrate=8 * S, frames=fr[:n1], in_off=k % 16, out_off=(3 * k) % 16) for k, fr in enumerate(streams)]
    first, host1 = E.call(E.DeviceMemory(pctx), specs, n1), E.call(E.HostMemory(), specs, n1)
    specs = [dict(sp, frames=fr[n1:], state=f["state"].tobytes()) for sp, fr, f in zip(specs, streams, first)]
    second, host2 = E.call(E.DeviceMemory(pctx), specs, n2), E.call(E.HostMemory(), specs, n2)
    for k, (w1, w2) in enumerate(wants):
        assert E.same(first[k], host1[k]) and E.same(second[k], host2[k]), (S, k, second[k]["result"], host2[k]["result"])
        assert (first[k]["out"] == w1[0]).all() and first[k]["result"].tobytes() == w1[1].tobytes(), (S, k)
        assert (second[k]["out"] == w2[0]).all() and second[k]["result"].tobytes() == w2[1].tobytes(), (S, k)
    assert E.counts_of(second[-1]["result"])["frames_overlapping"] == 1


@pytest.mark.gpu
def test_gpu_fec_chien_search_every_position_every_lane(pctx):
    """7. 204 rows with one error each, at every codeword position in turn; rows whose eight roots are all one lane's, and rows
    whose eight roots are eight lanes', all 12 rows of a frame at once"""
    sts = chien_streams()
    n = max(len(st["frames"]) for st in sts.values())
    specs = [dict(bitrate=st["bitrate"], frames=T.padded([st], n)[0]["frames"], out_off=off, in_off=3) for st, off in zip(sts.values(), (0, 2))]
    got, host = E.call(E.DeviceMemory(pctx), specs, n), E.call(E.HostMemory(), specs, n)
    for (name, st), g, h in zip(sts.items(), got, host):
        want = fec_want(name, st)
        assert E.same(g, h), (name, g["result"], h["result"])
        assert (g["out"][:len(want[0])] == want[0]).all(), name
        mine, ref = E.counts_of(g["result"]), E.counts_of(want[1])
        assert {k: mine[k] for k in F.COUNTERS[2:]} == {k: ref[k] for k in F.COUNTERS[2:]}, (name, mine, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SPLIT_SLOTS)
def test_gpu_fec_frame_split_between_out_and_state(pctx, S):
    """8. every place p = 1 .. 102 at which the boundary between d_out and the new state record can fall inside an FEC frame, an
    entry each, in three calls back to back with the state on the device; twice over: d_out and out_stride on 4 bytes (the
    correct kernel loads words) and off them (bytes)"""
    D = F.delay(8 * S)
    streams, wants = split_streams(S), split_wants(S)
    im = Image()
    specs = [dict(bitrate=8 * S, frames=fr, **lay) for lay in (dict(out_off=4 * (S % 4)), dict(out_off=1, out_stride=24 * S + 2, in_off=2)) for fr in streams]
    calls = [FecCall(im, specs, D)]
    for k in (1, 2):
        calls.append(FecCall(im, specs, D, frames_at=[L["frames"] for L in calls[0].lay], first=k * D, states=[L["sout"] for L in calls[-1].lay]))
    img = im.run(pctx, [c.call() for c in calls])
    for k, c in enumerate(calls):
        for e, g in enumerate(c.read(img)):
            want = wants[e % 102][k]
            assert (g["out"] == want[0]).all() and g["result"].tobytes() == want[1].tobytes(), (S, e, k)


@pytest.mark.gpu
def test_gpu_fec_tally_beyond_one_wave_of_frames(pctx):
    """9. 66 accepted frames in one entry, their counts all different (0 .. 8 errors, data and parity), summed by the tally's
    lane-stride loop; an entry of two frames beside it, whose surplus workgroups exit"""
    sts = tally_streams()
    n = len(sts["many"]["frames"])
    specs = [dict(bitrate=512, frames=T.padded([st], n)[0]["frames"], out_stride=1536 + extra) for st, extra in zip(sts.values(), (0, 5))]
    got, host = E.call(E.DeviceMemory(pctx), specs, n), E.call(E.HostMemory(), specs, n)
    for (name, st), g, h in zip(sts.items(), got, host):
        want = fec_want("tally " + name, st)
        assert E.same(g, h), (name, g["result"], h["result"])
        assert (g["out"][:len(want[0])] == want[0]).all(), name
        mine, ref = E.counts_of(g["result"]), E.counts_of(want[1])
        assert {k: mine[k] for k in F.COUNTERS[2:]} == {k: ref[k] for k in F.COUNTERS[2:]}, (name, mine, ref)
    assert E.counts_of(got[0]["result"])["frames"] == 66 and all(E.counts_of(got[0]["result"])[k] > 0 for k in F.COUNTERS[6:])


def stage_fec_specs():
    names = [n for n in E.STREAM_NAMES if n != "beyond"]
    base = {name: sp for name, sp in zip(E.STREAM_NAMES, E.all_specs(110))}
    return [dict(base[n], out_stride=3 * base[n]["bitrate"] + 3 * (k % 2)) for k in range(10) for n in names]


def stage_slides_specs():
    names = [n for n in T.STREAM_NAMES if len(T.streams()[n]["frames"]) <= 23][:13]
    return T.padded([T.spec_of(T.streams()[n], stride=3 * T.streams()[n]["bitrate"] + 3 * (k % 2)) for k in range(10) for n in names], 110)


@pytest.mark.gpu
def test_gpu_stage_area_small_large_small(built):
    """10. one stage area per context and call kind, grown behind a stream synchronise: a call of 2 entries x 4 frames, one of
    130 entries x 110 frames enqueued behind it, then the first again, nothing waiting in between; for the FEC call and for
    the slides call.  Every call's outputs equal the host twin's (the images), and the two small calls gave the same"""
    from conftest import make_ctx
    for kind in ("fec", "slides"):
        ctx = make_ctx()                                              # a context of its own: its stage areas have not grown yet
        im = Image()
        if kind == "fec":
            specs = stage_fec_specs()
            calls = [FecCall(im, specs[3:5], 4), FecCall(im, specs, 110), FecCall(im, specs[3:5], 4)]
        else:
            specs = stage_slides_specs()
            calls = [SlidesCall(im, specs[:2], 4), SlidesCall(im, specs, 110), SlidesCall(im, specs[:2], 4)]
        try:
            img = im.run(ctx, [c.call() for c in calls])
        finally:
            ctx.close()
        small, large, again = [c.read(img) for c in calls]
        assert len(large) == 130
        for a, b in zip(small, again):
            assert a["result"].tobytes() == b["result"].tobytes() and a["state"].tobytes() == b["state"].tobytes(), kind
            assert (a["out"] == b["out"]).all() if kind == "fec" else (a["arena"] == b["arena"]).all() and T.strip(a["slides"]) == T.strip(b["slides"]), kind
        if kind == "fec":
            assert sum(E.counts_of(g["result"])["frames"] for g in large) >= 130 and all(E.counts_of(g["result"])["cifs"] == 4 for g in small)
        else:
            assert sum(len(g["slides"]) for g in large) >= 60 and all(int(g["result"]["cifs"][0]) == 4 for g in small)
