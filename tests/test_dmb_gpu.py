"""T-DMB stream-mode sub-channels on the device: dabgpu_dmb_follow_dev held bit for bit to the host twin (and through it, or
directly, to tests/dmb_reference.py) -- packets, records, result, and the whole state record -- at the smallest shapes where
device code can be wrong and the host twin cannot: several entries of different bit rates in one table, more packets than one
wave and one chunk of the continuity launch hold, rows at a stride and off every boundary, packets whose gather straddles the
carried bytes and the call's rows, calls that emit nothing, two locks in one call.  Streams and helpers are tests/test_dmb.py's."""
import numpy as np
import pytest

import dabgpu
import dmb_reference as R
from test_dmb import (DEFER_CUTS, DEFER_ROOMS, FILL, RES, assert_is_reference, assert_same_stream, check_deferral, check_refusals,
                      continuity_packets, deferral_case, host_call, make_stream, noisy, ref_stream, run_stream, sprinkle)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dctx(built):
    from conftest import make_ctx
    c = make_ctx(None, max_frames=64)
    yield c
    c.close()


def dev_call_on(ctx, pad=0, offset=0):
    """host_call's twin on the device; rows `pad` bytes apart beyond the frame, the first `offset` bytes off a 16-byte boundary"""
    import torch

    def call(items, n_cifs):
        full = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        entries, keep = [], []
        for it in items:
            fb = 3 * it["bitrate"]
            m = it.get("capacity", dabgpu.dmb_max_packets(it["bitrate"], n_cifs))
            rows = np.full((max(n_cifs, 1), fb + pad), 0x47, np.uint8)           # (sync bytes in the gap: they must not be read)
            rows[:n_cifs, :fb] = it["frames"]
            d_in = torch.cat([torch.zeros(offset, dtype=torch.uint8), torch.from_numpy(rows.reshape(-1))]).cuda()
            a = dict(ts=full(max(m, 1) * 188), records=full(max(m, 1) * 16), result=full(80), state=full(dabgpu.dmb_state_bytes()),
                     state_in=None if it.get("state") is None else torch.from_numpy(np.ascontiguousarray(it["state"])).cuda(), d_in=d_in)
            keep.append(a)
            entries.append(dabgpu.DmbEntry(d_in.data_ptr() + offset if n_cifs else None, fb + pad, it["bitrate"], m, a["ts"].data_ptr(),
                                           a["records"].data_ptr(), None if a["state_in"] is None else a["state_in"].data_ptr(),
                                           a["state"].data_ptr(), a["result"].data_ptr()))
        ctx.dmb_follow_dev(entries, n_cifs)
        ctx.sync()
        return [{k: a[k].cpu().numpy() for k in ("ts", "records", "result", "state")} for a in keep]
    return call


def assert_call_is_host(got, want, what=""):
    for k in ("result", "records", "ts", "state"):
        if got[k].tobytes() != want[k].tobytes():
            bad = np.nonzero(got[k] != want[k])[0]
            pytest.fail("%s %s differs at bytes %s (%d in all): %s / %s" % (what, k, bad[:8], bad.size, got["result"].view(RES), want["result"].view(RES)))


@pytest.fixture(scope="module")
def three_streams():
    """8 kbit/s (a packet spans 9 frames and more), 136 and 544 kbit/s (1200 packets in 150 frames), every kind of packet"""
    return [(kbps, noisy(kbps, 150, 40 + kbps)) for kbps in (8, 136, 544)]


def test_three_entries_in_one_table(dctx, three_streams):
    """one table, calls of 140, 0, 9 and 1 frames: the first holds more than 256 packets of one entry (the chunk seam of the
    continuity launch, four waves of packets) and 1 packet of another; the later ones gather across the carried bytes"""
    dev = dev_call_on(dctx, pad=37, offset=3)
    states_d, states_h, at = [None] * 3, [None] * 3, 0
    emitted = np.zeros(3, int)
    for n in (140, 0, 9, 1):
        items = lambda states: [dict(bitrate=k, frames=f[at:at + n], state=s) for (k, f), s in zip(three_streams, states)]
        got, want = dev(items(states_d), n), host_call(items(states_h), n)
        for i in range(3):
            assert_call_is_host(got[i], want[i], "call of %d, entry %d" % (n, i))
            emitted[i] += int(want[i]["result"].view(RES)[0]["packets_emitted"])
        states_d, states_h, at = [g["state"] for g in got], [w["state"] for w in want], at + n
        if n == 140:
            assert emitted[0] == 1 and emitted[2] > 1024
    assert (emitted > [1, 280, 1150]).all()
    for (kbps, frames), s in zip(three_streams, states_d):                 # and the census against the reference
        census = dabgpu.dmb_state_census(s, kbps)
        assert [[int(e[k]) for k in ("pid", "packets", "discontinuities", "duplicates", "scrambled")] for e in census] == ref_stream(kbps, frames)["census"]


def test_calls_that_emit_nothing(dctx):
    frames = noisy(8, 100, 3)                                              # 2400 bytes: a lock, no complete packet
    dev = dev_call_on(dctx)
    got = run_stream(dev, 8, frames, [0, 60, 0, 40])
    assert_same_stream(got, run_stream(host_call, 8, frames, [0, 60, 0, 40]))
    assert got["counts"]["locks"] == 1 and got["counts"]["packets_emitted"] == 0 and got["counts"]["locked"] == 1


def test_cut_invariance_on_the_device(dctx):
    frames = noisy(136, 45, 77)
    dev = dev_call_on(dctx, pad=5, offset=1)
    whole, pieces = run_stream(dev, 136, frames), run_stream(dev, 136, frames, [7, 1, 20, 3, 14])
    assert_same_stream(pieces, whole)
    assert_same_stream(whole, run_stream(host_call, 136, frames))
    assert_is_reference(whole, ref_stream(136, frames), 136)


def test_undersized_buffers_defer_on_the_device(dctx):
    """rooms of 3, 0, 5, 10, 64, 2, 10, 0 and 64 packets for calls of 7, 1, 0, 20, 3, 14, 0, 0 and 0 frames: every call's buffers
    and state record are the host twin's, and the stream is that of the run with room for everything"""
    dev = dev_call_on(dctx, pad=5, offset=1)
    small, full, frames = deferral_case(dev)
    check_deferral(small, full)
    want = run_stream(host_call, 136, frames, DEFER_CUTS, rooms=DEFER_ROOMS)
    for i, (g, w) in enumerate(zip(small["calls"], want["calls"])):
        assert_call_is_host(g, w, "call %d" % i)
    # and beyond the record's 64 places packets are lost and counted, as on the host
    big = noisy(544, 20, 5)
    lost_d, lost_h = (run_stream(c, 544, big, [20, 0, 0], rooms=[10, 50, 50]) for c in (dev_call_on(dctx), host_call))
    assert_same_stream(lost_d, lost_h)
    assert lost_d["counts"]["packets_lost"] > 60 and lost_d["counts"]["packets_emitted"] == 74


def test_foreign_state_is_a_fresh_start_on_the_device(dctx):
    frames = noisy(136, 20, 9)
    dev = dev_call_on(dctx)
    fresh = run_stream(host_call, 136, frames)
    for state in (np.zeros(dabgpu.dmb_state_bytes(), np.uint8), np.full(dabgpu.dmb_state_bytes(), 0xA5, np.uint8)):
        assert_same_stream(run_stream(dev, 136, frames, state=state), fresh)


def test_burst_and_an_uncorrectable_packet(dctx):
    rng = np.random.default_rng(96)

    def burst(stream):
        stream[204 * 30 + 20:204 * 30 + 116] ^= rng.integers(1, 256, 96, dtype=np.uint8)
    frames = make_stream(136, 40, 4, coded_edit=lambda coded: sprinkle(rng, coded, [60], 11), stream_edit=burst)[0]
    got = run_stream(dev_call_on(dctx), 136, frames)
    assert_same_stream(got, run_stream(host_call, 136, frames))
    assert_is_reference(got, ref_stream(136, frames), 136)
    c = got["counts"]
    assert (c["packets_corrected"], c["packets_uncorrectable"], c["bytes_corrected"] + c["parity_bytes_corrected"]) == (12, 1, 96)
    bad = got["records"]["status"] == dabgpu.DMB_UNCORRECTABLE
    assert (got["ts"][bad, 1] & 0x80).all()


def test_two_locks_in_one_call(dctx):
    """a frame is missing: the lock is lost after 8 misses and another phase locks, inside one call and across calls"""
    frames = make_stream(128, 60, 13)[0]
    gone = np.concatenate([frames[:25], frames[26:]])
    dev = dev_call_on(dctx, pad=3, offset=2)
    got = run_stream(dev, 128, gone)
    assert_same_stream(got, run_stream(host_call, 128, gone))
    assert_is_reference(got, ref_stream(128, gone), 128)
    c = got["counts"]
    assert (c["locks"], c["lock_losses"], c["packets_dropped"], c["phase"]) == (2, 1, 11, 24)
    assert_same_stream(run_stream(dev, 128, gone, [26, 3, 30]), got)


def test_false_lock_first(dctx):
    def plant(s):
        for k in range(5):
            s[10 + 204 * k] = 0x47
    frames = make_stream(136, 30, 12, preamble=300, stream_edit=plant)[0]
    got = run_stream(dev_call_on(dctx), 136, frames)
    assert_same_stream(got, run_stream(host_call, 136, frames))
    assert (got["counts"]["locks"], got["counts"]["lock_losses"], got["counts"]["packets_dropped"]) == (2, 1, 8)


def test_continuity_across_the_chunk_seam(dctx):
    """every continuity rule with the packets of the PID on both sides of emitted packet 256 (a chunk of the continuity launch
    is 256 packets, a wave 64), and more PIDs than the census holds, first seen on both sides of it"""
    rules, disc, dup = continuity_packets()
    rules = rules[6:26]
    g = R.TsGenerator(31, pids=tuple(range(0x40, 0x40 + 20)), null_every=0)
    h = R.TsGenerator(32, pids=tuple(range(0x60, 0x60 + 20)), null_every=0)
    head = [g.next(pid=0x40 + i % 20) for i in range(4 + 256 - 9)]       # emitted packets start at packet 4
    tail = [h.next(pid=0x60 + i % 20) for i in range(R.packets_for(544, 40))]
    packets = np.stack(head + list(rules) + tail)
    broken = len(head) + 17
    assert (packets[broken, 3] & 15) == 13
    rng = np.random.default_rng(5)
    frames = make_stream(544, 40, packets=packets, coded_edit=lambda coded: sprinkle(rng, coded, [broken], 12))[0]
    got = run_stream(dev_call_on(dctx), 544, frames)
    assert_same_stream(got, run_stream(host_call, 544, frames))
    assert_is_reference(got, ref_stream(544, frames), 544)
    c = got["counts"]
    assert c["packets_emitted"] > 300 and (c["discontinuities"], c["duplicates"], c["pids"], c["pids_overflowed"]) == (disc, dup, 32, 11)
    assert int(got["records"]["pid"][255]) == 0x100 and int(got["records"]["pid"][256]) == 0x100
    assert_same_stream(run_stream(dev_call_on(dctx), 544, frames, [20, 20]), got)


def test_device_call_refuses(dctx):
    import torch
    frames = noisy(136, 4, 3)
    full = lambda n, v=FILL: torch.full((n,), v, dtype=torch.uint8, device="cuda")
    buffers = dict(d_in=torch.from_numpy(frames.reshape(-1).copy()).cuda(), d_ts=full(188 * 16), d_records=full(16 * 16),
                   d_state_in=full(dabgpu.dmb_state_bytes() + 16, 0), d_state_out=full(dabgpu.dmb_state_bytes() + 16), d_result=full(96))

    def follow(entries, n):
        dctx.dmb_follow_dev(entries, n)
        dctx.sync()
    check_refusals(follow, lambda b: b.data_ptr(), buffers, lambda b: b.cpu().numpy())


def test_end_to_end_through_the_eti_writer_and_reader(dctx):
    """the test transmitter's logical frames through dabgpu_eti_frames_dev and dabgpu_eti_read_dev, then the DMB call on the
    reader's rows: the packets the reference receiver finds on the frames themselves.  40 CIFs: the reader's 15 CIFs of FIC
    delay, a lock after 816 bytes and some 60 packets at 136 kbit/s."""
    import torch
    from test_eti import run_eti
    from test_eti_read import make_fibs
    frames, packets, _ = make_stream(136, 40, 61)
    streams = [(5, dabgpu.subchannel(0, 136, level=3))]
    fib, ok = make_fibs(np.random.default_rng(1), 40)
    eti, _, _ = run_eti(dctx, streams, fib[None], ok[None], [frames.reshape(1, 40, 408)])
    _, _, outs, _, result, _ = dctx.eti_read(torch.from_numpy(eti.reshape(1, -1)).cuda(), streams)
    assert int(result.cpu().numpy().view(dabgpu.ETI_READ_RESULT_DTYPE).reshape(-1)[0]["rows"]) == 40
    ts, records, res, state = dctx.dmb_follow(outs[0][:, :40], 136)
    res = res.cpu().numpy().view(RES).reshape(-1)[0]
    ref = ref_stream(136, frames)
    m = int(res["packets_emitted"])
    assert m == ref["counts"]["packets_emitted"] > 50 and int(res["packets_clean"]) == m
    assert ts.cpu().numpy()[0, :m].tobytes() == ref["ts"].tobytes() == packets[4:4 + m].tobytes()
    assert records.cpu().numpy()[0, :m].tobytes() == ref["records"].astype(dabgpu.DMB_RECORD_DTYPE).tobytes()
    # and the next call goes on from the state the first returned
    again = dctx.dmb_follow(outs[0][:, :0], 136, state)
    assert again[3].cpu().numpy().tobytes() == state.cpu().numpy().tobytes()
