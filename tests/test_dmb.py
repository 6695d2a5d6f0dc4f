"""T-DMB stream-mode sub-channels (include/dabgpu.h, "T-DMB"; include/dabgpu_dmb.h) on the CPU: the host twin
dabgpu_dmb_follow_host held byte for byte to tests/dmb_reference.py (the contract in plain Python, both interleavers as banks
of FIFOs) -- packets, records, counters, census -- and to itself across cuts (packets, records, census and the state record).
Outputs start out as 0xEE so that what a call must not write is compared too.  tests/test_dmb_gpu.py holds the device call to
the host twin with the helpers of this file."""
import os
import subprocess

import numpy as np
import pytest

import dabgpu
import dmb_reference as R
import packet_fec_reference as F
from conftest import ROOT

FILL = 0xEE
REC, RES = dabgpu.DMB_RECORD_DTYPE, dabgpu.DMB_RESULT_DTYPE
END_FIELDS = ("locked", "phase", "pids", "pids_overflowed", "packets_deferred")
SUMMED = dabgpu.DMB_COUNTERS + ("packets_lost",)


def aligned(n, fill=FILL):
    raw = np.full(n + 16, fill, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n]


# ------------------------------------------------------------------ streams
def make_stream(bitrate, n_frames, seed=1, packets=None, coded_edit=None, stream_edit=None, preamble=0, gen=None):
    """-> (frames [n_frames][3 * bitrate], the TS packets sent, the byte stream): packets from a seeded generator (or given),
    encoded, optionally damaged as codewords, interleaved, optionally behind `preamble` bytes of 0x00 and damaged as a
    stream, cut into frames"""
    need = R.packets_for(bitrate, n_frames)
    if packets is None:
        packets = (gen or R.TsGenerator(seed)).packets(need)
    assert len(packets) >= need
    coded = R.encode(packets)
    if coded_edit:
        coded_edit(coded)
    stream = np.concatenate([np.zeros(preamble, np.uint8), R.interleave(coded)])
    if stream_edit:
        stream_edit(stream)
    return R.to_frames(stream, bitrate)[:n_frames], packets, stream


def sprinkle(rng, coded, rows, n_errors):
    for r in rows:
        pos = rng.choice(204, n_errors, replace=False)
        coded[r, pos] ^= rng.integers(1, 256, n_errors, dtype=np.uint8)


# ------------------------------------------------------------------ running a call, and a stream as calls
def host_call(items, n_cifs):
    """items: dicts(bitrate, frames [n_cifs][>= 3 * bitrate] uint8 (a view may have a larger row stride), state or None) ->
    dicts(ts, records, result, state): whole buffers, FILL where nothing was written"""
    entries, keep = [], []
    for it in items:
        m = it.get("capacity", dabgpu.dmb_max_packets(it["bitrate"], n_cifs))
        fr = it["frames"]
        a = dict(ts=aligned(max(m, 1) * 188), records=aligned(max(m, 1) * 16), result=aligned(80), state=aligned(dabgpu.dmb_state_bytes()),
                 state_in=None if it.get("state") is None else aligned(dabgpu.dmb_state_bytes()))
        if a["state_in"] is not None:
            a["state_in"][:] = it["state"]
        keep.append((a, fr))
        entries.append(dabgpu.DmbEntry(fr.ctypes.data if n_cifs else None, fr.strides[0] if n_cifs else 3 * it["bitrate"], it["bitrate"], m,
                                       a["ts"].ctypes.data, a["records"].ctypes.data,
                                       None if a["state_in"] is None else a["state_in"].ctypes.data, a["state"].ctypes.data, a["result"].ctypes.data))
    dabgpu.dmb_follow_host(entries, n_cifs)
    return [dict(ts=a["ts"].copy(), records=a["records"].copy(), result=a["result"].copy(), state=a["state"].copy()) for a, _ in keep]


def run_stream(call, bitrate, frames, cuts=None, state=None, rooms=None):
    """the frames through `call` in calls of cuts[0], cuts[1], ... frames (None: one call), with room for rooms[i] packets in
    call i (None: dmb_max_packets, which holds everything) -> dict(ts [m][188], records REC [m], counts: the calls' counters
    summed and the last call's end fields, state, calls: each call's output)"""
    cuts = [len(frames)] if cuts is None else list(cuts)
    assert sum(cuts) == len(frames)
    ts, rec, counts, at, calls = [], [], dict.fromkeys(SUMMED, 0), 0, []
    for i, n in enumerate(cuts):
        item = dict(bitrate=bitrate, frames=frames[at:at + n], state=state)
        if rooms is not None and rooms[i] is not None:
            item["capacity"] = rooms[i]
        room = item.get("capacity", dabgpu.dmb_max_packets(bitrate, n))
        out = call([item], n)[0]
        at += n
        res = out["result"].view(RES)[0]
        m = int(res["packets_emitted"])
        assert 0 <= m <= room
        assert (out["ts"][m * 188:] == FILL).all() and (out["records"][m * 16:] == FILL).all(), "written beyond the emitted packets"
        ts.append(out["ts"][:m * 188].reshape(m, 188))
        rec.append(out["records"][:m * 16].view(REC))
        for k in SUMMED:
            counts[k] += int(res[k])
        for k in END_FIELDS:
            counts[k] = int(res[k])
        state = out["state"]
        calls.append(out)
    return dict(ts=np.concatenate(ts), records=np.concatenate(rec), counts=counts, state=state, calls=calls)


def ref_stream(bitrate, frames, cuts=None):
    cuts = [len(frames)] if cuts is None else list(cuts)
    rx, ts, rec, counts, at = R.Receiver(bitrate), [], [], dict.fromkeys(R.COUNTERS, 0), 0
    for n in cuts:
        t, r, c = rx.call(frames[at:at + n])
        at += n
        ts.append(t)
        rec.append(r)
        for k in R.COUNTERS:
            counts[k] += c[k]
        for k in END_FIELDS[:4]:
            counts[k] = c[k]
    counts["packets_deferred"] = counts["packets_lost"] = 0              # (the reference has room for everything, always)
    return dict(ts=np.concatenate(ts), records=np.concatenate(rec), counts=counts, census=rx.census)


def assert_is_reference(got, ref, bitrate, what=""):
    assert got["counts"] == ref["counts"], what
    assert got["ts"].tobytes() == ref["ts"].tobytes(), what
    assert got["records"].tobytes() == ref["records"].astype(REC).tobytes(), what
    census = dabgpu.dmb_state_census(got["state"], bitrate)
    assert [[int(e[k]) for k in ("pid", "packets", "discontinuities", "duplicates", "scrambled")] for e in census] == [list(map(int, e)) for e in ref["census"]], what


def assert_same_stream(a, b, what=""):
    assert a["counts"] == b["counts"], what
    assert a["ts"].tobytes() == b["ts"].tobytes(), what
    assert a["records"].tobytes() == b["records"].tobytes(), what
    assert a["state"].tobytes() == b["state"].tobytes(), what


def noisy(bitrate, n_frames, seed):
    """a stream with every kind of packet: clean, 1 .. 8 errors, a few beyond the bound"""
    rng = np.random.default_rng(seed)

    def edit(coded):
        rows = rng.permutation(np.arange(2, len(coded)))[:len(coded) // 3]
        for i, r in enumerate(rows):
            sprinkle(rng, coded, [r], 1 + i % 10)
    return make_stream(bitrate, n_frames, seed, coded_edit=edit)[0]


# ------------------------------------------------------------------ the contract's constants and sizes
def test_sizes_and_exports(built):
    assert dabgpu.dmb_state_bytes() == 24816 and dabgpu.DSCTY_MPEG2_TS == 24 and dabgpu.DMB_DEFER_ROOM == 64
    assert dabgpu.dmb_max_packets(8, 0) == 64 and dabgpu.dmb_max_packets(8, 9) == 64 + 2 and dabgpu.dmb_max_packets(544, 16) == 64 + 128
    assert dabgpu.dmb_max_packets(1824, 1) == 64 + 27
    for bad in ((0, 1), (12, 1), (1832, 1), (8, -1)):
        with pytest.raises(ValueError):
            dabgpu.dmb_max_packets(*bad)
    assert dabgpu.lib().dabgpu_abi_version() == 6


def test_encoder_and_interleaver_of_the_reference(built):
    """the test transmitter itself: codewords have zero syndromes, and the FIFO bank delays branch j by 204 j"""
    pk = R.TsGenerator(3).packets(30)
    coded = R.encode(pk)
    assert not F.syndromes(coded).any() and (coded[:, :188] == pk).all()
    y = R.interleave(coded)
    for n, i in ((0, 0), (3, 5), (7, 11), (10, 203), (12, 100)):
        assert y[204 * n + 204 * (i % 12) + i] == coded[n, i]


# ------------------------------------------------------------------ equality with the reference
@pytest.mark.parametrize("bitrate,n_frames", [(8, 420), (136, 40), (544, 12), (1824, 5)])
def test_host_twin_is_the_reference(built, bitrate, n_frames):
    """3 R mod 204 is 24, 0 (408 = 2 x 204), 0 (1632 = 8 x 204) and 168; packets of every status"""
    frames = noisy(bitrate, n_frames, bitrate)
    got, ref = run_stream(host_call, bitrate, frames), ref_stream(bitrate, frames)
    assert_is_reference(got, ref, bitrate)
    c = got["counts"]
    assert c["locks"] == 1 and c["packets_emitted"] > 5 and c["packets_corrected"] > 0 and c["packets_uncorrectable"] > 0 and c["phase"] == 0


@pytest.mark.parametrize("bitrate", [128, 1824])
def test_in_stride_and_unaligned_rows(built, bitrate):
    frames = noisy(bitrate, 24 if bitrate == 128 else 4, 5)
    wide = np.full((len(frames), 3 * bitrate + 37), 0x47, np.uint8)      # (sync bytes in the gap: they must not be read)
    flat = np.full(wide.size + 3, 0x47, np.uint8)
    view = flat[3:].reshape(wide.shape)
    view[:, :3 * bitrate] = frames
    a = run_stream(host_call, bitrate, frames)
    b = run_stream(host_call, bitrate, view[:, :3 * bitrate])
    assert_same_stream(a, b)


# ------------------------------------------------------------------ cut invariance
@pytest.mark.parametrize("bitrate,n_frames", [(8, 500), (136, 45)])
def test_cut_invariance(built, bitrate, n_frames):
    frames = noisy(bitrate, n_frames, 77)
    whole = run_stream(host_call, bitrate, frames)
    assert_is_reference(whole, ref_stream(bitrate, frames), bitrate)
    pattern = [1, 2, 0, 3, 7, 0, 0, 1, 11]
    cuts, left = [], n_frames
    while left:
        n = min(pattern[len(cuts) % len(pattern)], left)
        cuts.append(n)
        left -= n
    cuts.append(0)
    pieces = run_stream(host_call, bitrate, frames, cuts)
    assert_same_stream(pieces, whole, "cuts %s" % cuts)
    assert_is_reference(pieces, ref_stream(bitrate, frames, cuts), bitrate)
    # a call of no frames on a state record changes nothing but the counters of the call
    again = host_call([dict(bitrate=bitrate, frames=frames[:0], state=whole["state"])], 0)[0]
    assert again["state"].tobytes() == whole["state"].tobytes() and (again["ts"] == FILL).all()
    r = again["result"].view(RES)[0]
    assert all(int(r[k]) == 0 for k in SUMMED) and int(r["locked"]) == 1


# ------------------------------------------------------------------ undersized buffers: deferral
DEFER_CUTS = [7, 1, 0, 20, 3, 14, 0, 0, 0]
DEFER_ROOMS = [3, 0, 5, 10, 64, 2, 10, 0, 64]


def deferral_case(call, bitrate=136, n_frames=45, seed=77):
    """-> (the stream through `call` with rooms too small for what the calls bring, the same cuts with room for everything)"""
    frames = noisy(bitrate, n_frames, seed)
    return run_stream(call, bitrate, frames, DEFER_CUTS, rooms=DEFER_ROOMS), run_stream(call, bitrate, frames, DEFER_CUTS), frames


def check_deferral(small, full):
    """packets, records, the sums of the counters and the whole final state record are those of the run with room for everything;
    packets were held back on the way, none was lost, and each call wrote no more than it had room for"""
    assert_same_stream(small, full)
    held = [int(c["result"].view(RES)[0]["packets_deferred"]) for c in small["calls"]]
    emitted = [int(c["result"].view(RES)[0]["packets_emitted"]) for c in small["calls"]]
    assert max(held) >= 20 and held[-1] == 0 and small["counts"]["packets_lost"] == 0 and max(held) <= dabgpu.DMB_DEFER_ROOM
    assert all(e <= r for e, r in zip(emitted, DEFER_ROOMS)) and emitted != [int(c["result"].view(RES)[0]["packets_emitted"]) for c in full["calls"]]
    assert emitted[7] == 0 and emitted[6] == 10 and held[7] == held[6] > 0     # a call with no room and no frames moves nothing


def test_undersized_buffers_defer(built):
    small, full, frames = deferral_case(host_call)
    check_deferral(small, full)
    assert_is_reference(small, ref_stream(136, frames), 136)
    assert full["counts"]["discontinuities"] > 0 and full["counts"]["packets_uncorrectable"] > 0     # (continuity is judged at emission)


def test_packets_beyond_the_deferred_room_are_lost_and_counted(built):
    frames = noisy(544, 20, 5)
    full = run_stream(host_call, 544, frames)
    n = full["counts"]["packets_emitted"]
    small = run_stream(host_call, 544, frames, [20, 0, 0], rooms=[10, 50, 50])
    c = small["counts"]
    assert n > 140 and (c["packets_emitted"], c["packets_lost"], c["packets_deferred"]) == (10 + 50 + 14, n - 74, 0)
    assert small["ts"].tobytes() == full["ts"][:74].tobytes() and small["records"].tobytes() == full["records"][:74].tobytes()


def test_foreign_state_is_a_fresh_start(built):
    frames = noisy(136, 20, 9)
    fresh = run_stream(host_call, 136, frames)
    other = run_stream(host_call, 128, noisy(128, 20, 9))["state"]       # a record of another bit rate
    for state in (np.zeros(dabgpu.dmb_state_bytes(), np.uint8), np.full(dabgpu.dmb_state_bytes(), 0xA5, np.uint8), other):
        assert_same_stream(run_stream(host_call, 136, frames, state=state), fresh)


# ------------------------------------------------------------------ error patterns the reference alone decides
def test_eight_errors_are_corrected(built):
    rng = np.random.default_rng(8)
    rows = list(range(6, 60, 3))
    frames = make_stream(136, 40, 8, coded_edit=lambda coded: sprinkle(rng, coded, rows, 8))[0]
    got = run_stream(host_call, 136, frames)
    assert_is_reference(got, ref_stream(136, frames), 136)
    c = got["counts"]
    assert c["packets_corrected"] == len(rows) and c["packets_uncorrectable"] == 0
    assert c["bytes_corrected"] + c["parity_bytes_corrected"] == 8 * len(rows)


def test_nine_errors_are_uncorrectable(built):
    """nine errors lie beyond the bound: the packet goes out as received with the transport_error_indicator set.  A pattern
    that happens to lie within distance 8 of ANOTHER codeword is a miscorrection by definition; the reference says which
    patterns are, those are taken out, and no more than 1 in 20 may be."""
    rng = np.random.default_rng(9)
    rows = list(range(6, 126, 3))
    discarded = []

    def edit(coded):
        clean = coded.copy()
        sprinkle(rng, coded, rows, 9)
        _, verdicts = F.correct_rows(coded[rows])
        for r, v in zip(rows, verdicts):
            if v != -1:
                discarded.append(r)
                coded[r] = clean[r]
    frames, packets, _ = make_stream(136, 70, 9, coded_edit=edit)
    assert len(rows) == 40 and len(discarded) * 20 <= len(rows), "miscorrecting patterns: %s" % discarded
    got = run_stream(host_call, 136, frames)
    assert_is_reference(got, ref_stream(136, frames), 136)
    kept = len(rows) - len(discarded)
    assert got["counts"]["packets_uncorrectable"] == kept and got["counts"]["packets_corrected"] == 0
    bad = got["records"]["status"] == dabgpu.DMB_UNCORRECTABLE
    assert bad.sum() == kept and (got["ts"][bad, 1] & 0x80).all() and not (got["ts"][~bad, 1] & 0x80).any()


@pytest.mark.parametrize("length,corrected,uncorrectable", [(96, 12, 0), (108, 0, 12)])
def test_bursts(built, length, corrected, uncorrectable):
    """a burst inside one 204-byte slot spreads over 12 packets, length / 12 bytes each"""
    rng = np.random.default_rng(length)

    def edit(stream):
        stream[204 * 30 + 20:204 * 30 + 20 + length] ^= rng.integers(1, 256, length, dtype=np.uint8)
    frames = make_stream(136, 40, 4, stream_edit=edit)[0]
    got = run_stream(host_call, 136, frames)
    assert_is_reference(got, ref_stream(136, frames), 136)
    c = got["counts"]
    assert (c["packets_corrected"], c["packets_uncorrectable"]) == (corrected, uncorrectable)
    assert c["bytes_corrected"] + c["parity_bytes_corrected"] == (length if corrected else 0)
    bad = got["records"]["status"] == dabgpu.DMB_UNCORRECTABLE
    assert (got["ts"][bad, 1] & 0x80).all()


# ------------------------------------------------------------------ sync
def plant(stream, first, n):
    for k in range(n):
        stream[first + 204 * k] = 0x47


def test_four_false_sync_bytes_do_not_lock(built):
    frames = make_stream(136, 30, 11, preamble=300, stream_edit=lambda s: plant(s, 10, 4))[0]
    got = run_stream(host_call, 136, frames)
    assert_is_reference(got, ref_stream(136, frames), 136)
    c = got["counts"]
    assert (c["locks"], c["lock_losses"], c["packets_dropped"], c["phase"]) == (1, 0, 0, 300 % 204)
    assert int(got["records"]["position"][0]) == 300 + 4 * 204


def test_five_false_sync_bytes_lock_first(built):
    """the false phase reaches a run of 5 at 10 + 4 x 204 = 826, before the true one (300 + 816); it is lost 8 misses later and
    the true phase, whose run counter went on counting, locks at its next position"""
    frames = make_stream(136, 30, 12, preamble=300, stream_edit=lambda s: plant(s, 10, 5))[0]
    got = run_stream(host_call, 136, frames)
    assert_is_reference(got, ref_stream(136, frames), 136)
    c = got["counts"]
    assert (c["locks"], c["lock_losses"], c["packets_dropped"], c["phase"]) == (2, 1, 8, 300 % 204)
    lost_at = 826 + 8 * 204
    assert int(got["records"]["position"][0]) == 300 + 204 * -(-(lost_at + 1 - 300) // 204)


def test_a_lost_frame_moves_the_phase(built):
    """128 kbit/s: 384 bytes a frame, 384 mod 204 = 180.  One frame missing: 8 misses, the lock is lost, 11 packets dropped,
    and the new phase locks.  One frame zeroed: fewer than 8 sync bytes in a row are gone, the lock holds."""
    frames = make_stream(128, 60, 13)[0]
    gone = np.concatenate([frames[:25], frames[26:]])
    got = run_stream(host_call, 128, gone)
    assert_is_reference(got, ref_stream(128, gone), 128)
    c = got["counts"]
    assert (c["locks"], c["lock_losses"], c["packets_dropped"], c["phase"]) == (2, 1, 11, (204 - 180) % 204)
    cuts = [5, 20, 1, 7, 0, 26]
    assert_same_stream(run_stream(host_call, 128, gone, cuts), got)
    zeroed = frames.copy()
    zeroed[25] = 0
    got = run_stream(host_call, 128, zeroed)
    assert_is_reference(got, ref_stream(128, zeroed), 128)
    c = got["counts"]
    assert (c["locks"], c["lock_losses"], c["packets_dropped"]) == (1, 0, 0) and c["packets_uncorrectable"] > 0


def test_seven_damaged_sync_bytes_hold_the_lock(built):
    def edit(stream):
        for k in range(20, 27):
            stream[204 * k] = 0x00
    frames, packets, _ = make_stream(136, 40, 14, stream_edit=edit)
    got = run_stream(host_call, 136, frames)
    assert_is_reference(got, ref_stream(136, frames), 136)
    c = got["counts"]
    assert (c["locks"], c["lock_losses"], c["packets_corrected"], c["bytes_corrected"]) == (1, 0, 7, 7)
    assert (got["ts"][:, 0] == 0x47).all() and got["ts"].tobytes() == packets[4:4 + len(got["ts"])].tobytes()


def test_eight_damaged_sync_bytes_lose_it(built):
    def edit(stream):
        for k in range(20, 28):
            stream[204 * k] = 0x00
    frames = make_stream(136, 40, 15, stream_edit=edit)[0]
    got = run_stream(host_call, 136, frames)
    assert_is_reference(got, ref_stream(136, frames), 136)
    c = got["counts"]
    assert (c["locks"], c["lock_losses"], c["packets_dropped"], c["phase"]) == (2, 1, 11, 0)


# ------------------------------------------------------------------ continuity and census
def continuity_packets():
    """-> (packets, expected discontinuities, duplicates): every rule once on PID 0x100 between fillers of PID 0x200"""
    g = R.TsGenerator(21, pids=(0x200,), null_every=0)
    P = 0x100
    out = [g.next() for _ in range(6)]
    out += [R.ts_packet(P, 3, b"a"), R.ts_packet(P, 4, b"b")]                       # in order
    out += [R.ts_packet(P, 4, b"b")]                                                 # the same counter: a duplicate
    out += [R.ts_packet(P, 4, b"b")]                                                 # and again: every repetition counts
    out += [g.next(), R.ts_packet(P, 7, b"c")]                                       # 5 and 6 missing: a discontinuity
    out += [R.ts_packet(P, 7, afc=2)]                                                # no payload, the counter stands: in order
    out += [R.ts_packet(P, 9, afc=2)]                                                # no payload, the counter moved: a discontinuity
    out += [R.ts_packet(P, 2, b"d", afc=3, af=bytes([0x80]))]                        # discontinuity_indicator: exempt
    out += [R.ts_packet(P, 3, b"e", afc=3, af=b"")]                                  # an adaptation field of length 0 exempts nothing: in order
    out += [R.ts_packet(P, 9, b"f", afc=3, af=b"")]                                  # ... and here a discontinuity
    out += [R.ts_packet(R.NULL_PID, 5), R.ts_packet(R.NULL_PID, 9)]                  # null packets are exempt
    out += [R.ts_packet(P, 10, b"g", tsc=2)]                                         # in order, scrambled
    out += [g.next() for _ in range(3)]
    out += [R.ts_packet(P, 13, b"h")]                                                # BROKEN below: takes no part
    out += [R.ts_packet(P, 11, b"i")]                                                # in order after 10
    out += [g.next() for _ in range(R.packets_for(136, 24))]
    return np.stack(out), 3, 2


def test_every_continuity_rule(built):
    packets, disc, dup = continuity_packets()
    broken = int(np.nonzero((packets[:, 2] == 0x00) & (packets[:, 1] == 0x01) & ((packets[:, 3] & 15) == 13))[0][0])
    rng = np.random.default_rng(5)
    frames = make_stream(136, 24, packets=packets, coded_edit=lambda coded: sprinkle(rng, coded, [broken], 12))[0]
    got = run_stream(host_call, 136, frames)
    ref = ref_stream(136, frames)
    assert_is_reference(got, ref, 136)
    assert got["counts"]["packets_uncorrectable"] == 1
    assert (got["counts"]["discontinuities"], got["counts"]["duplicates"]) == (disc, dup)
    census = {int(e["pid"]): e for e in dabgpu.dmb_state_census(got["state"], 136)}
    assert [int(census[0x100][k]) for k in ("discontinuities", "duplicates", "scrambled")] == [disc, dup, 1]
    assert int(census[0x200]["discontinuities"]) == 0 and int(census[R.NULL_PID]["packets"]) == 2
    # the previous packet of a PID across every call boundary
    cuts = [1] * len(frames)
    assert_same_stream(run_stream(host_call, 136, frames, cuts), got)


def test_more_than_32_pids(built):
    g = R.TsGenerator(22, pids=tuple(range(0x40, 0x40 + 40)), null_every=0)
    packets = np.stack([g.next(pid=0x40 + (i * 7) % 40) for i in range(R.packets_for(136, 40))])
    frames = make_stream(136, 40, packets=packets)[0]
    got = run_stream(host_call, 136, frames)
    assert_is_reference(got, ref_stream(136, frames), 136)
    assert (got["counts"]["pids"], got["counts"]["pids_overflowed"], got["counts"]["discontinuities"]) == (32, 8, 0)
    assert_same_stream(run_stream(host_call, 136, frames, [9, 1, 0, 30]), got)


# ------------------------------------------------------------------ what the calls refuse
def refused_entries(entry_of):
    """(what, entry, n_cifs) for every refusal of the header's list; entry_of(**changes) makes the entry"""
    yield "n_cifs < 0", entry_of(), -1
    yield "n_cifs > 2^16", entry_of(), (1 << 16) + 1
    for kbps in (0, 4, 12, 1832, -8):
        yield "bit rate %d" % kbps, entry_of(bitrate_kbps=kbps), 4
    yield "short stride", entry_of(in_stride=3 * 136 - 1), 4
    yield "no d_in", entry_of(d_in=None), 4
    yield "negative room", entry_of(max_packets=-1), 4
    yield "no d_ts", entry_of(d_ts=None), 4
    yield "no d_records", entry_of(d_records=None), 4
    yield "no d_state_out", entry_of(d_state_out=None), 4
    yield "no d_result", entry_of(d_result=None), 4
    for f in ("d_ts", "d_records", "d_state_in", "d_state_out"):
        yield f + " off 16", entry_of(**{f: +8}), 4
    yield "d_result off 4", entry_of(d_result=+2), 4
    yield "state_out is state_in", entry_of(d_state_out="d_state_in"), 4
    yield "state_out overlaps state_in", entry_of(d_state_out=("d_state_in", 16)), 4


def check_refusals(follow, addr, buffers, read_back):
    """buffers: name -> buffer of the good entry; addr(buffer) its address; read_back(buffer) -> numpy"""
    def entry_of(**changes):
        f = dict(d_in=addr(buffers["d_in"]), in_stride=3 * 136, bitrate_kbps=136, max_packets=dabgpu.dmb_max_packets(136, 4),
                 d_ts=addr(buffers["d_ts"]), d_records=addr(buffers["d_records"]), d_state_in=addr(buffers["d_state_in"]),
                 d_state_out=addr(buffers["d_state_out"]), d_result=addr(buffers["d_result"]))
        for k, v in changes.items():
            if isinstance(v, str):
                f[k] = f[v]
            elif isinstance(v, tuple):
                f[k] = f[v[0]] + v[1]
            elif isinstance(v, int) and k.startswith("d_"):
                f[k] = f[k] + v
            else:
                f[k] = v
        return dabgpu.DmbEntry(*[f[n] for n, _ in dabgpu.DmbEntry._fields_])
    follow([entry_of()], 4)                                                # the good entry is taken
    before = {k: read_back(b).copy() for k, b in buffers.items()}
    for what, entry, n in refused_entries(entry_of):
        with pytest.raises(dabgpu.DabGpuError) as err:
            follow([entry_of(), entry], n)
        assert err.value.status == -1, what                                 # DABGPU_ERR_ARG
        for k, b in buffers.items():
            assert read_back(b).tobytes() == before[k].tobytes(), "%s: %s written" % (what, k)


def test_host_call_refuses(built):
    frames = noisy(136, 4, 3)
    buffers = dict(d_in=frames, d_ts=aligned(188 * 16), d_records=aligned(16 * 16), d_state_in=aligned(dabgpu.dmb_state_bytes() + 16, 0),
                   d_state_out=aligned(dabgpu.dmb_state_bytes() + 16), d_result=aligned(96))
    check_refusals(dabgpu.dmb_follow_host, lambda b: b.ctypes.data, buffers, lambda b: b)
    with pytest.raises(dabgpu.DabGpuError):
        dabgpu.dmb_follow_host([], -1)
    dabgpu.dmb_follow_host([], 0)


# ------------------------------------------------------------------ the header alone, under sanitizers
def test_fuzz_program_under_sanitizers(built, tmp_path):
    """tests/dmb_fuzz.cpp: the header alone, under AddressSanitizer and UBSan, on random bytes with sync bytes sown in, whole
    and in random cuts, and on hostile state records."""
    exe = tmp_path / "dmb_fuzz"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "dmb_fuzz.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), "60"], text=True)
    assert "dmb_fuzz ok" in out, out
