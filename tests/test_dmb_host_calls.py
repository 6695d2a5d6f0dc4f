"""The two host-only calls beside the T-DMB follow call: dabgpu_fig_stream_components (FIG 0/2 TMId 1 joined to FIG 0/1, on
FIBs made as tests/test_dabplus_follow.py makes them) and dabgpu_ts_programs (PAT and PMT sections out of TS packets, built
here bit by bit with a bitwise CRC-32/MPEG-2)."""
import ctypes as C

import numpy as np
import pytest

import dabgpu
import dmb_reference as R
from dabgpu import synth

ARG, CAPACITY = -1, -6


def fields(comps):
    return [(c.sid, c.subchid, c.start_address, c.dscty, c.primary, c.ca) for c in comps]


def stream_fibs():
    B = synth._bits
    sub = synth.fig0_1([{"id": 1, "start": 300, "option": 0, "level": 3, "size": 48}, {"id": 2, "start": 0, "uep_index": 17},
                        {"id": 3, "start": 100, "option": 1, "level": 3, "size": 36}, {"id": 9, "start": 500, "option": 2, "level": 3, "size": 48},
                        {"id": 10, "start": 600, "option": 0, "level": 3, "size": 6}])
    fig2 = lambda body, **kw: synth.fig0(2, body, **{"cn": 0, "oe": 0, "pd": 0, **kw})
    figs = [
        sub,
        # P/D = 1: a packet-mode component (TMId 3), a T-DMB stream (TMId 1, DSCTy 24, secondary, CA) and a DAB+ one (TMId 0)
        fig2(B((0xE1C00123, 32), (0, 1), (0, 3), (3, 4)) + B((3, 2), (0x123, 12), (0, 1), (0, 1)) +
             B((1, 2), (24, 6), (10, 6), (0, 1), (1, 1)) + B((0, 2), (63, 6), (3, 6), (0, 1), (0, 1)), pd=1),
        # P/D = 0: another DSCTy on sub-channel 1 (reported, not judged); sub-channel 10 again (listed once); a stream on a
        # sub-channel nobody announced (20) and one whose sub-channel has a reserved option (9)
        fig2(B((0xC001, 16), (0, 1), (0, 3), (4, 4)) + B((1, 2), (5, 6), (1, 6), (1, 1), (0, 1)) + B((1, 2), (24, 6), (10, 6), (1, 1), (0, 1)) +
             B((1, 2), (24, 6), (20, 6), (1, 1), (0, 1)) + B((1, 2), (24, 6), (9, 6), (1, 1), (0, 1))),
        # the next configuration and another ensemble's services do not count
        fig2(B((0xC003, 16), (0, 1), (0, 3), (1, 4)) + B((1, 2), (24, 6), (2, 6), (1, 1), (0, 1)), cn=1),
        fig2(B((0xC004, 16), (0, 1), (0, 3), (1, 4)) + B((1, 2), (24, 6), (2, 6), (1, 1), (0, 1)), oe=1),
    ]
    fibs = synth.pack_fibs(figs)
    filler = synth.pack_fibs([synth.fig0_0(0xC181, 0)])
    return np.concatenate([fibs] + [filler] * (12 - len(fibs)))[None], figs, filler


def test_fig_stream_components(built):
    fib, figs, filler = stream_fibs()
    ok = np.ones((1, 12), np.uint8)
    want = [(0xC001, 1, 300, 5, 1, 0), (0xE1C00123, 10, 600, dabgpu.DSCTY_MPEG2_TS, 0, 1)]
    assert fields(dabgpu.fig_stream_components(fib, ok)) == want
    # the join: every start address is one of dabgpu_fig_subchannels' entries
    starts = {sc.start_address: sc for sc in dabgpu.fig_subchannels(fib, ok)}
    assert all(w[2] in starts for w in want) and starts[600].bitrate_kbps == 8
    # the sub-channels announced in the LAST FIB: the join does not depend on the order
    late = np.ascontiguousarray(fib[:, list(range(1, 12)) + [0]])
    assert fields(dabgpu.fig_stream_components(late, ok)) == want
    # FIBs whose CRC failed say nothing; without FIG 0/1 nothing can be joined
    assert dabgpu.fig_stream_components(fib, np.zeros((1, 12), np.uint8)) == []
    none = np.concatenate([synth.pack_fibs(figs[1:])] + [filler] * 12)[:12][None]
    assert dabgpu.fig_stream_components(none, ok) == []
    # audio and packet components are not stream components, and the other way round
    assert [c.subchid for c in dabgpu.fig_audio_components(fib, ok)] == [3]


def test_fig_stream_components_capacity(built):
    fib, _, _ = stream_fibs()
    fib = np.ascontiguousarray(fib)
    ok = np.ones((1, 12), np.uint8)
    L = dabgpu.lib()
    arr = (dabgpu.StreamComponent * 3)()
    for a in arr:
        a.subchid = -7
    n = C.c_int(-1)
    assert L.dabgpu_fig_stream_components(fib.ctypes.data, ok.ctypes.data, 1, arr, 1, C.byref(n)) == CAPACITY and n.value == 2
    assert all(a.subchid == -7 for a in arr)
    assert L.dabgpu_fig_stream_components(fib.ctypes.data, ok.ctypes.data, 1, None, 0, C.byref(n)) == CAPACITY and n.value == 2
    assert L.dabgpu_fig_stream_components(fib.ctypes.data, ok.ctypes.data, 1, arr, 2, C.byref(n)) == 0 and [a.subchid for a in arr] == [1, 10, -7]
    with pytest.raises(dabgpu.DabGpuError) as err:
        dabgpu.fig_stream_components(fib, ok, max_out=1)
    assert err.value.status == CAPACITY
    assert L.dabgpu_fig_stream_components(None, ok.ctypes.data, 1, arr, 2, C.byref(n)) == ARG
    assert L.dabgpu_fig_stream_components(fib.ctypes.data, ok.ctypes.data, 1, None, 2, C.byref(n)) == ARG
    assert L.dabgpu_fig_stream_components(fib.ctypes.data, ok.ctypes.data, 1, arr, 2, None) == ARG


# ------------------------------------------------------------------ PSI
def crc32_mpeg2(data):
    """x^32 + x^26 + x^23 + x^22 + x^16 + x^12 + x^11 + x^10 + x^8 + x^7 + x^5 + x^4 + x^2 + x + 1, register all ones, bit by bit"""
    reg = 0xFFFFFFFF
    for byte in data:
        for bit in range(7, -1, -1):
            top = (reg >> 31) & 1
            reg = (reg << 1) & 0xFFFFFFFF
            if top ^ ((byte >> bit) & 1):
                reg ^= 0x04C11DB7
    return reg


def section(table_id, ext, body, current=1, version=3):
    n = 5 + len(body) + 4
    head = bytes([table_id, 0xB0 | (n >> 8), n & 0xFF, ext >> 8, ext & 0xFF, 0xC0 | (version << 1) | current, 0, 0])
    s = head + bytes(body)
    return s + crc32_mpeg2(s).to_bytes(4, "big")


def pat(ts_id, programs, **kw):
    return section(0, ts_id, b"".join(bytes([n >> 8, n & 0xFF, 0xE0 | (p >> 8), p & 0xFF]) for n, p in programs), **kw)


def pmt(number, pcr_pid, streams, program_info=b"", **kw):
    body = bytes([0xE0 | (pcr_pid >> 8), pcr_pid & 0xFF, 0xF0 | (len(program_info) >> 8), len(program_info) & 0xFF]) + program_info
    for st, pid, es_info in streams:
        body += bytes([st, 0xE0 | (pid >> 8), pid & 0xFF, 0xF0 | (len(es_info) >> 8), len(es_info) & 0xFF]) + es_info
    return section(2, number, body, **kw)


def packetize(pid, sections, cc0=0, lead=b""):
    """sections back to back into packets of one PID: pointer_field where a section starts, 0xFF stuffing at the end;
    `lead`: bytes of an earlier section that the first pointer_field skips"""
    data, out, cc = lead + b"".join(sections), [], cc0
    starts, at = [], len(lead)
    for s in sections:
        starts.append(at)
        at += len(s)
    pos = 0
    while pos < len(data):
        room = 184
        first = next((s for s in starts if s >= pos), None)
        pusi = first is not None and first - pos < room - 1
        if pusi:
            chunk = data[pos:pos + room - 1]
            payload = bytes([first - pos]) + chunk
        else:
            chunk = data[pos:pos + room]
            payload = chunk
        pos += len(chunk)
        out.append(R.ts_packet(pid, cc, payload, pusi=int(pusi)))
        cc = (cc + 1) & 15
    return out


def test_ts_programs(built):
    iod = bytes([0x1D, 4, 1, 2, 3, 4])
    long_info = bytes([0x05, 150]) + bytes(150)                            # makes the PMT span two packets
    streams = [(0x12, 0x111, bytes([0x1E, 2, 0, 1])), (0x12, 0x112, bytes([0x1E, 2, 0, 2])), (0x1B, 0x113, b""), (0x0F, 0x114, long_info)]
    p1 = pmt(1, 0x113, streams, program_info=iod)
    p2 = pmt(2, 0x1FFF, [(0x06, 0x120, b"")])
    assert len(p1) > 183 and len(p2) < 100
    g = R.TsGenerator(5, pids=(0x111, 0x113), null_every=3)
    packets = [g.next() for _ in range(3)]
    packets += packetize(0, [pat(0x4D42, [(0, 0x10), (1, 0x100), (2, 0x100), (3, 0x300)])])
    packets += [g.next()]
    pm = packetize(0x100, [p1, p2])                                        # programme 2's PMT begins inside packet 2
    assert len(pm) == 2
    packets += [pm[0], g.next(), R.ts_packet(0x100, 0, afc=2), pm[1]]      # a packet without payload does not break the section
    packets += [g.next() for _ in range(3)]
    info = dabgpu.ts_programs(np.stack(packets))
    assert (info.transport_stream_id, info.network_pid, info.n_programs, info.pat_sections, info.pmt_sections, info.crc_errors) == (0x4D42, 0x10, 3, 1, 2, 0)
    a, b, c = info.programs[0], info.programs[1], info.programs[2]
    assert (a.program_number, a.pmt_pid, a.pmt_seen, a.pcr_pid, a.iod_present, a.n_streams) == (1, 0x100, 1, 0x113, 1, 4)
    assert list(zip(a.stream_type[:4], a.stream_pid[:4])) == [(0x12, 0x111), (0x12, 0x112), (0x1B, 0x113), (0x0F, 0x114)]
    assert (b.program_number, b.pmt_seen, b.pcr_pid, b.iod_present, b.n_streams, b.stream_type[0], b.stream_pid[0]) == (2, 1, 0x1FFF, 0, 1, 6, 0x120)
    assert (c.program_number, c.pmt_pid, c.pmt_seen) == (3, 0x300, 0)


def test_ts_programs_damage(built):
    good = pat(7, [(1, 0x100)])
    bad = bytearray(pmt(1, 0x101, [(0x1B, 0x101, b"")]))
    bad[10] ^= 1                                                           # a section with a bad CRC is counted and ignored
    packets = packetize(0, [good]) + packetize(0x100, [bytes(bad)])
    info = dabgpu.ts_programs(np.stack(packets))
    assert (info.n_programs, info.pat_sections, info.pmt_sections, info.crc_errors, info.programs[0].pmt_seen) == (1, 1, 0, 1, 0)
    # the same section, sound, after it: taken.  A next (not current) PAT does not replace the current one
    packets += packetize(0x100, [pmt(1, 0x101, [(0x1B, 0x101, b"")])], cc0=1) + packetize(0, [pat(8, [(9, 0x900)], current=0)], cc0=1)
    info = dabgpu.ts_programs(np.stack(packets))
    assert (info.transport_stream_id, info.n_programs, info.pmt_sections, info.crc_errors, info.programs[0].pcr_pid) == (7, 1, 1, 1, 0x101)
    # a lost packet in the middle of a two-packet section (continuity counter jumps): no section, no CRC error
    long_pmt = pmt(1, 0x101, [(0x1B, 0x101, bytes([0x05, 200]) + bytes(200))])
    two = packetize(0x100, [long_pmt])
    assert len(two) == 2
    info = dabgpu.ts_programs(np.stack(packetize(0, [good]) + [two[0], R.ts_packet(0x100, 5, bytes(184))]))
    assert (info.pmt_sections, info.crc_errors) == (0, 0)
    # a packet with the transport_error_indicator set takes no part
    broken = two[1].copy()
    broken[1] |= 0x80
    info = dabgpu.ts_programs(np.stack(packetize(0, [good]) + [two[0], broken]))
    assert (info.pmt_sections, info.crc_errors) == (0, 0)
    # a section that starts behind the rest of an earlier one: the pointer_field skips it
    info = dabgpu.ts_programs(np.stack(packetize(0, [good], lead=bytes(range(1, 20)))))
    assert (info.transport_stream_id, info.pat_sections) == (7, 1)
    # nothing at all
    info = dabgpu.ts_programs(np.zeros((0, 188), np.uint8))
    assert (info.transport_stream_id, info.n_programs) == (-1, 0)
    assert dabgpu.lib().dabgpu_ts_programs(None, 1, C.byref(dabgpu.TsInfo())) == ARG
    assert dabgpu.lib().dabgpu_ts_programs(None, 0, None) == ARG
