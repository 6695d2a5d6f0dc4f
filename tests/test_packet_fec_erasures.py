"""RS(204,188) correction of packet-mode FEC frames with failed packet CRCs as erasures (dabgpu_packet_fec_erasures_dev,
dabgpu_packet_fec_erasures_host; the contract: include/dabgpu_packet_fec.h, "Erasures") against
tests/packet_fec_erasure_reference.py, which decodes by Euclid's algorithm on the modified syndromes and verifies every
correction by definition.  Each stream below is about one clause; its `counts` are asserted on the REFERENCE's result before
the code under test is held to it.  Every comparison is on bytes and integers.  See tests/README_packet_fec_erasures.md."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import packet_fec_erasure_reference as E
import packet_fec_reference as F
import packet_reference as R
import test_packet as T
import test_packet_fec as P
from conftest import ROOT
from test_device_asm import CSRC, kernel_metadata

ARG = -1
FILL, GAP = 0xA7, 64
ADDR = T.ADDR
RESULT_BYTES = 80
RATES = (8, 24, 40, 400, 512)                                          # S = 1, 3, 5, 50, 64; D = 102, 34, 21, 3, 2


# ------------------------------------------------------------------------------------------------ building streams
def frames_of(bitrate, packets, tables):
    """the packets in FEC frames, just long enough for `tables` of them to come out: their slots, then the delay"""
    S = bitrate // 8
    n = -(-103 * tables // S)
    fr = np.concatenate([synth.packet_fec_frames(bitrate, [packets], n_frames=n)[:n], synth.packet_frames(bitrate, [], n_frames=F.delay(bitrate))])
    flat = fr.reshape(-1, 24)
    for t in range(tables):                                            # table t lies at slots 103 t ..: what at() and wipe() count on
        assert [F.mark(flat[103 * t + 94 + i]) for i in range(9)] == list(range(9))
    return fr


def one_slot_packets(rng, n):
    return [synth.packet(ADDR, bytes(rng.integers(0, 256, 19, dtype=np.uint8)), 1, ci=k) for k in range(n)]


def clean_frames(bitrate, seed, tables=3):
    """every packet one slot: an overwritten packet is one suspect slot, two columns"""
    return frames_of(bitrate, one_slot_packets(np.random.default_rng(seed), 94 * tables), tables)


def wipe(frames, table, slots, rng):
    """whole one-slot packets overwritten: every one of the 24 bytes differs from what was sent, and the first says two slots
    or more, so the slot reads neither as a mark nor (but for a CRC of 2^-16) as a good packet"""
    flat = frames.reshape(-1, 24)
    for s in slots:
        old = flat[103 * table + s]
        assert old[0] >> 6 == 0
        new = old ^ rng.integers(1, 256, 24, dtype=np.uint8)
        if new[0] >> 6 == 0:
            new[0] ^= 0x40
        flat[103 * table + s] = new


def hit_parity(frames, table, per_row, rng):
    """per_row(r) errors in the parity columns of every row r of a table (the FEC packets carry no CRC: nothing is suspect)"""
    for r in range(12):
        P.hit(frames, table, r, [int(c) for c in rng.choice(np.arange(188, 204), per_row(r), replace=False)], rng=rng)


ALL_ROWS = (3, 4, 5, 6, 7, 8, 9, 12, 13, 14)                           # with the two CRC bytes: one byte in each of the twelve rows


def forge(frames, table, s, offsets, rng):
    """an error in a data column that no CRC shows: bytes of a one-slot packet damaged (byte o lies in row o % 12) and its CRC
    made to check again, which changes rows 10 and 11 as well: the packet is not suspect"""
    slot = frames.reshape(-1, 24)[103 * table + s]
    for o in offsets:
        assert 3 <= o < 22
        slot[o] ^= int(rng.integers(1, 256))
    c = R.crc(bytes(slot[:22]))
    assert (c >> 8) != slot[22] and (c & 0xFF) != slot[23]
    slot[22], slot[23] = c >> 8, c & 0xFF


def slot_of(frames, table, s):
    return frames.reshape(-1, 24)[103 * table + s]


def stream(bitrate, sent, received, **counts):
    return dict(bitrate=bitrate, sent=sent, frames=received, counts=counts)


def _streams():
    S = {}
    rng = np.random.default_rng(4202)

    # whole packets overwritten: 1 (the errors-only rule), 5 and 8 (step 3, e = 0), 9 (f = 18: left alone)
    sent = clean_frames(32, 1, tables=4)
    fr = sent.copy()
    lost = [(17,), (3, 20, 50, 77, 93), (0, 1, 11, 40, 41, 66, 80, 92), (2, 9, 10, 33, 47, 58, 71, 85, 90)]
    for t, slots in enumerate(lost):
        wipe(fr, t, slots, rng)
    S["slots"] = stream(32, sent, fr, frames=4, marks=36, rows_clean=0, rows_corrected=12, rows_erasure_corrected=24, rows_uncorrectable=12,
                        slots_suspect=23, frames_with_suspects=4, frames_beyond_erasures=1, erasure_other_bytes_corrected=0, parity_bytes_corrected=0)

    # erasures and errors elsewhere, in data and parity columns: f = 12 with one (2 + 12 = 14: step 3), f = 2 with six (eight
    # wrong bytes: the errors-only rule takes it first), f = 4 with five (10 + 4 = 14, nine wrong bytes: step 3), f = 14 with
    # one (beyond the margin: left alone)
    sent = clean_frames(32, 2, tables=4)
    fr = sent.copy()
    lost = [(5, 6, 30, 31, 60, 93), (44,), (12, 70), (1, 15, 29, 43, 57, 71, 85)]
    for t, slots in enumerate(lost):
        wipe(fr, t, slots, rng)
    forge(fr, 0, 50, (3, 4, 5, 6, 7, 8, 9), rng)                       # rows 3 .. 11 in the data, rows 0 .. 2 in the parity
    hit_parity(fr, 0, lambda r: int(r < 3), rng)
    forge(fr, 1, 20, ALL_ROWS, rng)
    hit_parity(fr, 1, lambda r: 5, rng)
    forge(fr, 2, 33, ALL_ROWS, rng)
    hit_parity(fr, 2, lambda r: 4, rng)
    hit_parity(fr, 3, lambda r: 1, rng)
    S["mixed"] = stream(32, sent, fr, frames=4, rows_clean=0, rows_corrected=12, rows_erasure_corrected=24, rows_uncorrectable=12,
                        slots_suspect=16, frames_with_suspects=4, frames_beyond_erasures=0, erasure_other_bytes_corrected=12 * 1 + 12 * 5)

    # table 0: five packets overwritten and one with a single damaged byte: 23 of its 24 erased bytes are right, the errata
    # values there are zero.  table 1: nine packets with only a CRC byte damaged (f = 18), five in row 10 and four in row 11:
    # the errors-only rule corrects them
    sent = clean_frames(32, 3, tables=2)
    fr = sent.copy()
    wipe(fr, 0, (8, 19, 33, 61, 88), rng)
    slot_of(fr, 0, 50)[7] ^= 0x21
    for k, s in enumerate((4, 14, 24, 34, 44, 54, 64, 74, 84)):
        slot_of(fr, 1, s)[22 + k % 2] ^= 0x80 >> (k % 8)
    S["one byte"] = stream(32, sent, fr, frames=2, rows_clean=10, rows_corrected=2, rows_erasure_corrected=12, rows_uncorrectable=0, bytes_corrected=9,
                           slots_suspect=15, frames_with_suspects=2, frames_beyond_erasures=1, erasure_other_bytes_corrected=0)

    # table 0: a packet of four slots (a whole logical frame) with one damaged byte; every inner slot begins with a length of
    # four slots, which does not fit: four suspect slots.  With four one-slot packets overwritten f = 16: eight wrong bytes in eleven rows (the errors-only rule)
    # and nine in the row of the damaged byte (step 3).  table 1: a damaged
    # length field in the last slot of a logical frame (step 2 of the scan) beside five overwritten packets
    prng = np.random.default_rng(4)
    payload = bytearray(prng.integers(0, 256, 91, dtype=np.uint8))
    for inner in (21, 45, 69):                                         # byte 24, 48, 72 of the packet
        payload[inner] = 0xC0
    pk = one_slot_packets(prng, 8) + [synth.packet(ADDR, bytes(payload), 4, ci=8)] + one_slot_packets(prng, 2 * 94 - 12)
    sent = frames_of(32, pk, 2)
    assert sent[2].tobytes() == pk[8]
    fr = sent.copy()
    slot_of(fr, 0, 10)[13] ^= 0x04
    wipe(fr, 0, (0, 37, 62, 91), rng)
    assert 103 % 4 == 3 and (103 + 4) % 4 == 3                         # slot 4 of table 1 is the last of its logical frame
    slot_of(fr, 1, 4)[0] |= 0x40
    wipe(fr, 1, (9, 22, 23, 56, 78), rng)
    S["long packets"] = stream(32, sent, fr, frames=2, rows_corrected=11, rows_erasure_corrected=13, rows_uncorrectable=0, slots_suspect=8 + 6,
                               frames_with_suspects=2, frames_beyond_erasures=0, erasure_other_bytes_corrected=0)

    # a damaged packet whose CRC checks again: not suspect.  Rows 5, 10 and 11 (the damaged byte and the two CRC bytes) have
    # an error outside E: beside f = 12 they are corrected as errors, beside f = 14 they are left alone
    sent = clean_frames(32, 5, tables=2)
    fr = sent.copy()
    for t, slots in enumerate([(7, 21, 35, 49, 63, 77), (7, 21, 35, 49, 63, 77, 91)]):
        wipe(fr, t, slots, rng)
        forge(fr, t, 55, (5,), rng)
    S["undetected"] = stream(32, sent, fr, frames=2, rows_clean=0, rows_corrected=0, rows_erasure_corrected=12 + 9, rows_uncorrectable=3,
                             slots_suspect=13, frames_with_suspects=2, erasure_other_bytes_corrected=3)

    # rows past the bound, 167 x 12 of them: f = 16 with 1 .. 3 errors elsewhere (step 3 with e = 0 gives the codeword that
    # agrees outside E: bytes change in suspect slots only), and e one over: f = 12 with two, f = 8 with four, f = 4 with six
    sent = clean_frames(512, 6, tables=167)
    fr = sent.copy()
    for t in range(167):
        f, k = [(16, None), (12, 2), (8, 4), (4, 6)][t % 4]
        slots = [int(s) for s in rng.choice(94, f // 2, replace=False)]
        wipe(fr, t, slots, rng)
        hit_parity(fr, t, (lambda r, t=t: 1 + (t // 4 + r) % 3) if k is None else (lambda r, k=k: k), rng)
    S["beyond"] = stream(512, sent, fr, frames=167, marks=9 * 167, rows_clean=0, rows_corrected=0, frames_with_suspects=167, frames_beyond_erasures=0,
                         rows_erasure_corrected=12 * 42, rows_uncorrectable=12 * 125, erasure_other_bytes_corrected=0)

    # bit rates: five overwritten packets in every FEC frame, spread over the logical frames the table lies in
    for rate in RATES:
        sent = clean_frames(rate, 10 + rate)
        fr = sent.copy()
        for t in range(3):
            wipe(fr, t, (2 + t, 30, 47 + 5 * t, 70, 93), rng)
        S["rate %d" % rate] = stream(rate, sent, fr, frames=3, marks=27, rows_clean=0, rows_corrected=0, rows_erasure_corrected=36, rows_uncorrectable=0,
                                     slots_suspect=15, frames_with_suspects=3, erasure_other_bytes_corrected=0)
    return S


STREAM_NAMES = ["slots", "mixed", "one byte", "long packets", "undetected", "beyond"] + ["rate %d" % r for r in RATES]
#: the streams of test_packet_fec.py on which the errors-only call leaves no row uncorrectable
SUPERSET_NAMES = ["rows", "two bad marks", "three bad marks", "counter 9", "mid-frame", "no fec"] + ["rate %d" % r for r in P.RATES]
STREAMS = None


def streams():
    global STREAMS
    if STREAMS is None:
        STREAMS = _streams()
        assert list(STREAMS) == STREAM_NAMES
    return STREAMS


_WANTS = {}


def wanted(name):
    """the reference's answer to a whole stream in one call: computed once, shared, left as it is"""
    if name not in _WANTS:
        st = streams()[name]
        out, counts = E.Receiver(st["bitrate"]).call(st["frames"])
        out.setflags(write=False)
        _WANTS[name] = (out, counts)
    return _WANTS[name]


# ------------------------------------------------------------------------------------------------ one call, on any memory
class HostMemory(P.HostMemory):
    def run(self, entries, n_cifs):
        dabgpu.packet_fec_erasures_host(entries, n_cifs)


class DeviceMemory(P.DeviceMemory):
    def run(self, entries, n_cifs):
        self.ctx.packet_fec_erasures_dev(entries, n_cifs)
        self.ctx.sync()


def call(mem, specs, n_cifs, mutate=None, refused=None):
    """test_packet_fec.call for the erasure pair: one call on buffers laid out in one allocation, every region between
    sentinel bytes; after the call nothing but the n_cifs output frames, state-out and the result may have changed (nothing at
    all for a refused call).  -> per entry dict(out [n_cifs][3 R], result, state)"""
    size, lay = 0, []

    def take(n):
        nonlocal size
        off = (size + GAP + 255) // 256 * 256
        size = off + n
        return off

    for sp in specs:
        fb, nb = 3 * sp["bitrate"], dabgpu.packet_fec_state_bytes(sp["bitrate"])
        lay.append(dict(fb=fb, nb=nb, stride=sp.get("stride", fb), ostride=sp.get("out_stride", fb),
                        frames=take(max(n_cifs, 1) * sp.get("stride", fb) + 16) + sp.get("in_off", 0),
                        out=take(max(n_cifs, 1) * sp.get("out_stride", fb) + 16) + sp.get("out_off", 0),
                        sin=take(nb) if sp.get("state") is not None else None, sout=take(nb), result=take(RESULT_BYTES)))
    img = np.full(size + GAP, FILL, np.uint8)
    for sp, L in zip(specs, lay):
        for k in range(n_cifs):
            img[L["frames"] + k * L["stride"]:L["frames"] + k * L["stride"] + L["fb"]] = sp["frames"][k]
        if L["sin"] is not None:
            img[L["sin"]:L["sin"] + L["nb"]] = np.frombuffer(bytes(sp["state"]), np.uint8)
    base = mem.load(img)
    assert base % 256 == 0
    entries = [dabgpu.PacketFecErasureEntry(base + L["frames"], L["stride"], sp["bitrate"], 0, base + L["out"], L["ostride"],
                                            base + L["sin"] if L["sin"] is not None else None, base + L["sout"], base + L["result"]) for sp, L in zip(specs, lay)]
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
        untouched[L["sout"]:L["sout"] + L["nb"]] = False
        untouched[L["result"]:L["result"] + RESULT_BYTES] = False
        rows = np.zeros((n_cifs, L["fb"]), np.uint8)
        for k in range(n_cifs):
            a = L["out"] + k * L["ostride"]
            untouched[a:a + L["fb"]] = False
            rows[k] = after[a:a + L["fb"]]
        out.append(dict(out=rows, result=after[L["result"]:L["result"] + RESULT_BYTES].copy().view(dabgpu.PACKET_FEC_ERASURE_RESULT_DTYPE),
                        state=after[L["sout"]:L["sout"] + L["nb"]].copy()))
    assert (after[untouched] == img[untouched]).all(), "bytes outside the outputs changed"
    return out


def run_cut(mem_of, st, cuts, first_state=None, **kw):
    """the stream in len(cuts) + 1 calls -> (output frames, summed counters, the last state record)"""
    edges = [0] + list(cuts) + [len(st["frames"])]
    state, outs, results = first_state, [], []
    for a, b in zip(edges[:-1], edges[1:]):
        got = call(mem_of(), [dict(bitrate=st["bitrate"], frames=st["frames"][a:b], state=state, **kw)], b - a)[0]
        outs.append(got["out"])
        results.append(got["result"])
        state = got["state"].tobytes()
    return np.concatenate(outs), E.total(results), state


def counts_of(rec):
    return {k: int(rec[k][0]) for k in E.COUNTERS}


def old_call(st):
    """the errors-only host call on a whole stream"""
    return P.call(P.HostMemory(), [dict(bitrate=st["bitrate"], frames=st["frames"])], len(st["frames"]))[0]


def data_slots(n_slots, phase=0):
    """which of a stream's slots lie in application data tables (the first table begins `phase` slots before slot 0)"""
    return (np.arange(n_slots) + phase) % 103 < 94


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_records_and_sizes(built, tmp_path):
    L = dabgpu.lib()
    for name in ("dabgpu_packet_fec_erasures_dev", "dabgpu_packet_fec_erasures_host"):
        assert name in dabgpu.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    dt = dabgpu.PACKET_FEC_ERASURE_RESULT_DTYPE
    assert dt.itemsize == RESULT_BYTES == E.RESULT_DTYPE.itemsize and dt.names == E.RESULT_DTYPE.names and dt.itemsize % 16 == 0
    assert dt.names[:12] == dabgpu.PACKET_FEC_RESULT_DTYPE.names
    assert [dt.fields[f][1] for f in dt.names[:12]] == [dabgpu.PACKET_FEC_RESULT_DTYPE.fields[f][1] for f in dt.names[:12]]
    assert hasattr(dabgpu.Context, "packet_fec_erasures_dev")
    # the binding's structure and the record against the header, as the C compiler lays them out; the entry's fields are
    # those of dabgpu_packet_fec_entry
    assert [(f, t) for f, t in dabgpu.PacketFecErasureEntry._fields_] == [(f, t) for f, t in dabgpu.PacketFecEntry._fields_]
    lines, want = ['#include <stdio.h>', '#include <stddef.h>', '#include "dabgpu.h"', 'int main(void) {'], []
    lines.append('  printf(" %zu", sizeof(dabgpu_packet_fec_erasure_entry));')
    lines += ['  printf(" %%zu", offsetof(dabgpu_packet_fec_erasure_entry, %s));' % f for f, _ in dabgpu.PacketFecErasureEntry._fields_]
    lines += ['  printf(" %%zu", offsetof(dabgpu_packet_fec_entry, %s));' % f for f, _ in dabgpu.PacketFecEntry._fields_]
    offs = [getattr(dabgpu.PacketFecErasureEntry, f).offset for f, _ in dabgpu.PacketFecErasureEntry._fields_]
    want += [C.sizeof(dabgpu.PacketFecErasureEntry)] + offs + offs
    lines.append('  printf(" %zu", sizeof(dabgpu_packet_fec_erasure_result));')
    lines += ['  printf(" %%zu", offsetof(dabgpu_packet_fec_erasure_result, %s));' % f for f in dt.names]
    want += [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ['  return 0; }']) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == want


def test_reference_decodes_what_the_definition_says_it_must():
    """the reference on its own: erasures at random columns with random (also zero) values, and errors elsewhere up to the
    bound, come back; one error more than the bound allows does not; nothing changes outside E without the bound"""
    rng = np.random.default_rng(19)
    rows = rng.integers(0, 256, (9, 188), dtype=np.uint8)
    cw = np.concatenate([rows, np.stack([synth.rs204_parity(r) for r in rows])], axis=1)
    for f in (2, 4, 8, 12, 14, 16):
        Ecols = sorted(int(c) for s in rng.choice(94, f // 2, replace=False) for c in (2 * s, 2 * s + 1))
        free = [c for c in range(204) if c not in Ecols]
        most = (14 - f) // 2 if f <= 12 else 0
        bad = cw.copy()
        bad[:, Ecols] = rng.integers(0, 256, (9, f), dtype=np.uint8)
        bad[0, Ecols[1:]] = cw[0, Ecols[1:]]                           # row 0: all but one of the erased bytes are right
        for i in range(9):
            for c in rng.choice(free, min(i, most), replace=False):
                bad[i, c] ^= rng.integers(1, 256)
        fixed, verdicts = E.correct_rows(bad, Ecols)
        assert (fixed == cw).all(), f
        over = cw.copy()
        over[:, Ecols] ^= rng.integers(1, 256, (9, f), dtype=np.uint8)
        for i in range(9):
            for c in rng.choice(free, max(most + 1, 9 - f) if f < 16 else 1, replace=False):
                over[i, c] ^= rng.integers(1, 256)
        fixed, verdicts = E.correct_rows(over, Ecols)
        outside = [c for c in range(204) if c not in Ecols]
        if f < 16:
            assert (fixed == over).all() and verdicts == [("unchanged",)] * 9, (f, verdicts)
        else:
            assert (fixed[:, outside] == over[:, outside]).all() and not F.syndromes(fixed).any() and all(v[0] == "erasures" and v[2] == 0 for v in verdicts)


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_host_equals_the_reference(built, name):
    """each stream in one call: the stream's own expectations on the REFERENCE's result first, then the host twin against it,
    byte for byte"""
    st = streams()[name]
    want, wc = wanted(name)
    ref = counts_of(wc)
    for key, v in st["counts"].items():
        assert ref[key] == v, (name, key, ref)
    D, S = F.delay(st["bitrate"]), st["bitrate"] // 8
    assert ref["cifs"] == len(st["frames"]) and ref["slots"] == S * len(st["frames"])
    assert ref["rows_clean"] + ref["rows_corrected"] + ref["rows_erasure_corrected"] + ref["rows_uncorrectable"] == 12 * ref["frames"]
    assert (want[:D] == np.frombuffer(synth.packet(0, b"", 1, fill=0) * S, np.uint8)).all()
    got = call(HostMemory(), [dict(bitrate=st["bitrate"], frames=st["frames"])], len(st["frames"]))[0]
    assert counts_of(got["result"]) == ref and got["result"].tobytes() == wc.tobytes(), (name, got["result"], wc)
    assert (got["out"] == want).all(), name
    n = len(st["frames"]) - D
    out, sent, raw = want[D:].reshape(-1, 24), st["sent"][:n].reshape(-1, 24), st["frames"][:n].reshape(-1, 24)
    data = data_slots(n * S)
    table = np.arange(n * S) // 103
    if name in ("one byte", "long packets") or name.startswith("rate"):
        assert (out[data] == sent[data]).all(), "the data as sent"
    if name == "slots":
        assert (out[data & (table < 3)] == sent[data & (table < 3)]).all() and (out[table == 3] == raw[table == 3]).all()
        assert ref["erased_bytes_changed"] > 13 * 24 - 12
    if name == "mixed":
        assert (out[data & (table < 3)] == sent[data & (table < 3)]).all() and (out[table == 3] == raw[table == 3]).all()
        assert ref["bytes_corrected"] + ref["parity_bytes_corrected"] >= 12 * 8 - 2
    if name == "one byte":
        assert ref["erased_bytes_changed"] <= 5 * 24 + 1
    if name == "undetected":
        rows = np.arange(24) % 12
        keep = np.isin(rows, (5, 10, 11))
        assert (out[data & (table == 0)] == sent[data & (table == 0)]).all()
        one = data & (table == 1)
        assert (out[one][:, ~keep] == sent[one][:, ~keep]).all() and (out[one][:, keep] == raw[one][:, keep]).all()


def test_the_errors_only_call_loses_what_erasures_recover(built):
    """`slots`: five and eight overwritten packets are twelve uncorrectable rows each for dabgpu_packet_fec_host (and nine, of
    course); the erasure call brings the first two back"""
    st = streams()["slots"]
    old = P.counts_of(old_call(st)["result"])
    assert old["frames"] == 4 and old["rows_corrected"] == 12 and old["rows_uncorrectable"] == 36 and old["rows_clean"] == 0
    new = counts_of(call(HostMemory(), [dict(bitrate=32, frames=st["frames"])], len(st["frames"]))[0]["result"])
    assert new["rows_corrected"] == 12 and new["rows_erasure_corrected"] == 24 and new["rows_uncorrectable"] == 12


@pytest.mark.parametrize("name", SUPERSET_NAMES)
def test_what_the_errors_only_call_corrects_is_corrected_identically(built, name):
    """every stream of test_packet_fec.py on which the errors-only call leaves no row uncorrectable: the output and the first
    twelve result words of the erasure call are that call's"""
    st = P.streams()[name]
    old = old_call(st)
    assert P.counts_of(old["result"])["rows_uncorrectable"] == 0
    new = call(HostMemory(), [dict(bitrate=st["bitrate"], frames=st["frames"])], len(st["frames"]))[0]
    assert (new["out"] == old["out"]).all() and new["result"].tobytes()[:48] == old["result"].tobytes(), name
    assert counts_of(new["result"])["rows_erasure_corrected"] == 0
    assert new["state"].tobytes()[64:] == old["state"].tobytes()[64:] and new["state"].tobytes()[:4] != old["state"].tobytes()[:4]


def test_rows_beyond_the_bound_are_decided_by_the_reference(built):
    """2004 rows past the bound.  The reference decides each, and the twin agreed byte for byte
    (test_host_equals_the_reference).  Here, on the reference's own result: no byte outside E changed anywhere (the seed shows
    no miscorrection outside E), and in the f = 16 frames every changed byte lies in a suspect slot"""
    st = streams()["beyond"]
    want, wc = wanted("beyond")
    ref = counts_of(wc)
    print("rows beyond the bound: %d taken by step 3 (all f = 16), %d uncorrectable, %d by the errors-only rule, of %d"
          % (ref["rows_erasure_corrected"], ref["rows_uncorrectable"], ref["rows_corrected"], 12 * ref["frames"]))
    assert ref["frames"] == 167 and ref["rows_corrected"] == 0 and ref["erasure_other_bytes_corrected"] == 0
    D, S = 2, 64
    n = len(st["frames"]) - D
    out, raw = want[D:].reshape(-1, 24), st["frames"][:n].reshape(-1, 24)
    suspect = np.concatenate([E.suspect_slots(f, S) for f in st["frames"][:n]])
    changed = (out != raw).any(axis=1)
    table = np.arange(n * S) // 103
    assert changed.any() and not (changed & ~suspect).any()
    assert not changed[table % 4 != 0].any() and changed[table % 4 == 0].sum() >= 42 * 8 - 4


CUT_NAMES = [n for n in STREAM_NAMES if n != "beyond"]


@pytest.mark.parametrize("name", CUT_NAMES)
def test_cut_into_two_calls_at_every_frame_boundary(built, name):
    """the result of a stream does not depend on where it is cut: two calls at every frame boundary (so every carried frame
    holds suspect slots of a straddling FEC frame at some cut), calls of no frame, and a run of short calls: output, summed
    counters and the last state record equal the uncut run's"""
    st = streams()[name]
    n = len(st["frames"])
    whole = run_cut(HostMemory, st, [])
    assert (whole[0] == wanted(name)[0]).all()
    for k in range(0, n + 1):
        got = run_cut(HostMemory, st, [k])
        assert (got[0] == whole[0]).all() and got[1] == whole[1] and got[2] == whole[2], (name, k)
    got = run_cut(HostMemory, st, [n // 3, n // 3, n // 3 + 1, n // 2, n // 2, n // 2])
    assert (got[0] == whole[0]).all() and got[1] == whole[1] and got[2] == whole[2]


def test_the_long_stream_cut_into_calls(built):
    st = streams()["beyond"]
    n = len(st["frames"])
    whole = run_cut(HostMemory, st, [])
    assert (whole[0] == wanted("beyond")[0]).all()
    for cuts in ([0], [1], [2, 3], [n // 2], [n // 2, n // 2 + 1], [n - 1], [n]):
        got = run_cut(HostMemory, st, cuts)
        assert (got[0] == whole[0]).all() and got[1] == whole[1] and got[2] == whole[2], cuts


def test_foreign_zero_and_errors_only_state_records_are_a_fresh_start(built):
    st = streams()["rate 40"]
    nb = dabgpu.packet_fec_state_bytes(40)
    whole = run_cut(HostMemory, st, [])
    k = 30                                                             # a cut with suspect slots in the carried frames
    first = call(HostMemory(), [dict(bitrate=40, frames=st["frames"][:k])], k)[0]["state"].tobytes()
    assert any(first[32:64]) and first[:4] == b"PFEE"
    old = P.call(P.HostMemory(), [dict(bitrate=40, frames=st["frames"][:k])], k)[0]["state"].tobytes()
    assert old[:4] == b"PFEC" and old[4:32] == first[4:32] and not any(old[32:64])
    spoiled = bytearray(first)
    spoiled[32 + 13] |= 0x40                                           # bit 110 of 105 carried slots: an unused position
    assert F.delay(40) * 5 == 105
    for state in (bytes(nb), bytes(np.random.default_rng(5).integers(0, 256, nb, dtype=np.uint8)), bytes([0xFF]) * nb, old, bytes(spoiled),
                  b"PFEC" + first[4:]):
        got = run_cut(HostMemory, st, [], first_state=state)
        assert (got[0] == whole[0]).all() and got[1] == whole[1] and got[2] == whole[2]
    # ... and a record of the erasure call is a fresh start for the errors-only call
    want = P.run_cut(P.HostMemory, st, [])
    got = P.run_cut(P.HostMemory, st, [], first_state=first)
    assert (got[0] == want[0]).all() and got[1] == want[1] and got[2] == want[2]
    # a record of this call and this bit rate is not: the stream goes on behind it
    cont = run_cut(HostMemory, dict(st, frames=st["frames"][k:]), [], first_state=first)
    assert (cont[0] == whole[0][k:]).all() and cont[2] == whole[2]
    # padding frames below stream frame 0 hold no suspect slot: a record that says so is none of this code's
    early = call(HostMemory(), [dict(bitrate=40, frames=st["frames"][:2])], 2)[0]["state"].tobytes()
    bad = bytearray(early)
    bad[32] |= 0x01
    a = call(HostMemory(), [dict(bitrate=40, frames=st["frames"], state=bytes(bad))], len(st["frames"]))[0]
    assert (a["out"] == whole[0]).all()


# ---- refusals
def refusal_specs():
    st = streams()["rate 40"]
    nb = dabgpu.packet_fec_state_bytes(40)
    return [dict(bitrate=40, frames=st["frames"], state=bytes(nb), stride=128, out_stride=130, in_off=3, out_off=7) for _ in range(3)], 6


def test_refusals_that_need_no_device(built):
    specs, n = refusal_specs()
    for m in P.BAD_ENTRIES:
        call(HostMemory(), specs, n, mutate=m, refused=ARG)
    L = dabgpu.lib()
    e = (dabgpu.PacketFecErasureEntry * 1)()
    host, dev = L.dabgpu_packet_fec_erasures_host, L.dabgpu_packet_fec_erasures_dev
    assert host(None, 1, 1) == ARG and host(e, -1, 1) == ARG and host(e, 1, -1) == ARG
    assert host(e, 1, (1 << 24) + 1) == ARG and dev(None, e, 1, 1, None) == ARG
    dabgpu.packet_fec_erasures_host([], 3)                             # nothing to do is not an error
    got = call(HostMemory(), specs, 0, mutate=lambda es: [setattr(x, "d_in", None) or setattr(x, "d_out", None) for x in es])
    assert all(counts_of(g["result"]) == dict.fromkeys(E.COUNTERS, 0) for g in got)


# ---- device code, sanitizers
def test_new_kernels_neither_spill_nor_use_scratch(built, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the device assembly cannot be checked")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "packet_fec_kernels.hip" in mk and "dabgpu_packet_fec_api.hip" in mk and "dabgpu_packet_fec_erasures.h" in mk
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    out = tmp_path / "packet_fec_kernels.s"
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "packet_fec_kernels.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    md = kernel_metadata(out.read_text())
    # the file holds both calls' kernels: this call's four, each once, and the errors-only call's four, and no others
    assert all(sum(k in name for name in md) == 1 for k in ("packet_fec_erasure_move_kernel", "packet_fec_erasure_accept_kernel",
                                                            "packet_fec_erasure_correct_kernel", "packet_fec_erasure_tally_kernel"))
    assert len(md) == 8 and all(sum(k in name for name in md) == 1 for k in ("packet_fec_move_kernel", "packet_fec_accept_kernel",
                                                                            "packet_fec_correct_kernel", "packet_fec_tally_kernel"))
    for k, v in md.items():
        print("%s: vgprs %s, sgprs %s, LDS %s bytes" % (k, v.get("vgpr_count"), v.get("sgpr_count"), v.get("group_segment_fixed_size")))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)


def test_erasure_fuzz_under_sanitizers(tmp_path):
    """tests/packet_fec_erasure_fuzz.cpp: random and damaged streams and random state records through process_erasures,
    every buffer a heap block of exactly its size; a stand-alone program built with the host compiler under AddressSanitizer
    and UBSan and run as a child process"""
    exe = str(tmp_path / "packet_fec_erasure_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "packet_fec_erasure_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "calls=2000" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = dict(kv.split("=") for kv in r.stdout.split())
    print(r.stdout)
    for key in ("frames", "clean", "corrected", "erasure_corrected", "uncorrectable", "suspect", "beyond", "fresh", "carried", "empty"):
        assert int(got[key]) > 0, (key, r.stdout)


# ---- the chain: FEC in front of the slides call
CHAIN_OBJECT = T.obj(0x612, 500, 41, b"erasures.png", 200)


def chain_frames():
    """32 kbit/s: one slide, carried once, in one-slot packets, behind it padding; in every FEC frame eight slots wiped"""
    pk = synth.packetise(CHAIN_OBJECT[2], ADDR, sizes=(1,))
    sent = np.concatenate([synth.packet_fec_frames(32, [pk], n_frames=52)[:52], synth.packet_frames(32, [], n_frames=F.delay(32))])
    assert 30 < len(pk) < 94
    raw = sent.copy()
    rng = np.random.default_rng(8)
    for s in (1, 4, 5, 11, 17, 22, 23, 29):                            # of the slide's packets
        P.wipe(raw, s, rng)
    for s in range(1, 9):                                              # behind the slide: two padding packets of four slots
        P.wipe(raw, 103 + s, rng)
    return sent, raw


def test_chain_erasures_then_slides_delivers_what_the_errors_only_call_loses(built):
    sent, raw = chain_frames()
    header, body = CHAIN_OBJECT[0], CHAIN_OBJECT[1]
    lost, lc = R.Receiver(1024, ADDR, 1).call(raw, 32, 2, 1024)       # the REFERENCE on the raw frames: the slide is lost
    assert lost == [] and int(lc["slots_bad"][0]) >= 8
    old = P.call(P.HostMemory(), [dict(bitrate=32, frames=raw)], len(raw))[0]
    assert P.counts_of(old["result"])["rows_uncorrectable"] == 24
    behind_old = P.slides_host(old["out"])
    assert T.strip(behind_old["slides"]) == [] and int(behind_old["result"]["slots_bad"][0]) >= 8
    fixed = call(HostMemory(), [dict(bitrate=32, frames=raw)], len(raw))[0]
    n = counts_of(fixed["result"])
    assert n["frames"] == 2 and n["rows_erasure_corrected"] == 24 and n["rows_uncorrectable"] == 0 and n["slots_suspect"] == 16
    got = P.slides_host(fixed["out"])
    assert T.strip(got["slides"]) == [(0x612, 2, 1, header, body)]
    assert int(got["result"]["slots_bad"][0]) == 0 and int(got["result"]["packets_fec"][0]) == 9 * 2


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


ALL_NAMES = STREAM_NAMES + ["chain"] + SUPERSET_NAMES


def stream_of(name, k):
    if k < len(STREAM_NAMES):
        return streams()[name]
    if name == "chain":
        return dict(bitrate=32, frames=chain_frames()[1])
    return P.streams()[name]


def all_specs(n_cifs):
    """every stream as one entry of one table, frames of 0xFF behind the shorter ones: in_stride and out_stride beyond 3 R and
    frames off their 16-byte and 4-byte boundaries by turns"""
    specs = []
    for e, name in enumerate(ALL_NAMES):
        st = stream_of(name, e)
        fr = st["frames"][:n_cifs]
        if len(fr) < n_cifs:
            fr = np.concatenate([fr, np.full((n_cifs - len(fr), fr.shape[1]), 0xFF, np.uint8)])
        specs.append(dict(bitrate=st["bitrate"], frames=fr, stride=3 * st["bitrate"] + [0, 2, 16, 5][e % 4], out_stride=3 * st["bitrate"] + [0, 16, 3, 4][(e // 2) % 4],
                          in_off=[0, 8, 4, 1, 13][e % 5], out_off=[0, 4, 0, 7, 16][(e + 1) % 5]))
    return specs


def same(g, h):
    return g["result"].tobytes() == h["result"].tobytes() and (g["out"] == h["out"]).all() and g["state"].tobytes() == h["state"].tobytes()


@pytest.fixture
def limit():
    """every GPU step under a time limit of its own: a step that hangs ends the whole run (nothing more is started on the
    device behind it) with the stacks of all threads"""
    import faulthandler
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.gpu
def test_gpu_every_stream_in_one_call(pctx, limit):
    """all streams in ONE call (rows of 0xFF behind the shorter streams): bit rates from 8 to 512, strides beyond 3 R, d_in and
    d_out off 16 and off 4 bytes: output, counters and state record equal the host call's byte for byte, and for three of the
    streams the reference's where the stream lies"""
    n = max(len(stream_of(name, e)["frames"]) for e, name in enumerate(ALL_NAMES))
    specs = all_specs(n)
    got = call(DeviceMemory(pctx), specs, n)
    host = call(HostMemory(), specs, n)
    for e, (name, g, h) in enumerate(zip(ALL_NAMES, got, host)):
        assert same(g, h), (name, g["result"], h["result"])
        if name in ("slots", "mixed", "rate 400"):                     # (the host twin is held to the reference for every stream on the CPU)
            want, wc = wanted(name)
            assert (g["out"][:len(want)] == want).all(), name
            ref, mine = counts_of(wc), counts_of(g["result"])
            skip = ("cifs", "slots", "slots_suspect")                  # (the rows of 0xFF behind the stream are slots, and suspect)
            assert {k: mine[k] for k in E.COUNTERS if k not in skip} == {k: ref[k] for k in E.COUNTERS if k not in skip}, name
    total = E.total([g["result"] for g in got])
    assert total["rows_erasure_corrected"] >= 600 and total["rows_corrected"] >= 200 and total["rows_uncorrectable"] >= 1500


@pytest.mark.gpu
@pytest.mark.parametrize("n_cifs", [0, 1, 7])
def test_gpu_short_calls(pctx, limit, n_cifs):
    """calls of 0, 1 and 7 logical frames, every entry, from a fresh start and from the state the host left after 30 frames"""
    specs = all_specs(n_cifs)
    got = call(DeviceMemory(pctx), specs, n_cifs)
    host = call(HostMemory(), specs, n_cifs)
    for name, g, h in zip(ALL_NAMES, got, host):
        assert same(g, h), name
    longer = all_specs(30 + n_cifs)
    first = call(HostMemory(), [dict(sp, frames=sp["frames"][:30]) for sp in longer], 30)
    later = [dict(sp, frames=sp["frames"][30:], state=f["state"].tobytes()) for sp, f in zip(longer, first)]
    got = call(DeviceMemory(pctx), later, n_cifs)
    host = call(HostMemory(), later, n_cifs)
    for name, g, h in zip(ALL_NAMES, got, host):
        assert same(g, h), name
    assert any(any(f["state"].tobytes()[32:64]) for f in first)        # suspect bits were carried in


@pytest.mark.gpu
def test_gpu_two_calls_back_to_back_with_the_state_on_the_device(pctx, limit):
    """every stream in two calls enqueued one behind the other, nothing waiting in between, cut where an FEC frame with suspect
    slots on both sides straddles the calls: the state record of the first is the second's input: output, summed counters and
    the last state equal the uncut host run's"""
    import torch
    bufs = {}
    for name in STREAM_NAMES:
        st = streams()[name]
        S = st["bitrate"] // 8
        n, nb, fb = len(st["frames"]), dabgpu.packet_fec_state_bytes(st["bitrate"]), 3 * st["bitrate"]
        # a cut inside a data table that has suspect slots on both sides of it
        sus = np.concatenate([E.suspect_slots(f, S) for f in st["frames"][:min(n, 4 * 103 // S + 1)]])
        cut = next(c for c in range(1, len(sus) // S) if 0 < c * S % 103 < 94 and sus[c * S - c * S % 103:c * S].any() and sus[c * S:c * S - c * S % 103 + 94].any())
        bufs[name] = dict(frames=torch.from_numpy(st["frames"]).cuda(), out=torch.full((n, fb), FILL, dtype=torch.uint8, device="cuda"), cut=cut,
                          states=torch.zeros((2, nb), dtype=torch.uint8, device="cuda"), results=torch.zeros((2, RESULT_BYTES), dtype=torch.uint8, device="cuda"))
    for k in range(2):
        for name in STREAM_NAMES:
            st, b = streams()[name], bufs[name]
            a, n_cifs = (b["cut"], len(st["frames"]) - b["cut"]) if k else (0, b["cut"])
            pctx.packet_fec_erasures_dev([dabgpu.PacketFecErasureEntry(b["frames"][a].data_ptr(), 3 * st["bitrate"], st["bitrate"], 0, b["out"][a].data_ptr(),
                                                                       3 * st["bitrate"], b["states"][0].data_ptr() if k else None, b["states"][k].data_ptr(),
                                                                       b["results"][k].data_ptr())], n_cifs)
    pctx.sync()
    for name in STREAM_NAMES:
        b, st = bufs[name], streams()[name]
        whole = run_cut(HostMemory, st, [])
        res = b["results"].cpu().numpy().view(dabgpu.PACKET_FEC_ERASURE_RESULT_DTYPE).reshape(2)
        assert (b["out"].cpu().numpy() == whole[0]).all(), name
        assert E.total([res[k:k + 1] for k in range(2)]) == whole[1], name
        assert b["states"][1].cpu().numpy().tobytes() == whole[2], name


@pytest.mark.gpu
def test_gpu_single_frame_calls_across_an_fec_frame(pctx, limit):
    """8 kbit/s, S = 1: 140 calls of one frame each (one slot), across the first FEC frame (five suspect slots, three of them
    behind slot 40) and into the second, the state ping-ponging on the device, nothing waiting in between"""
    import torch
    st = streams()["rate 8"]
    n, nb = 140, dabgpu.packet_fec_state_bytes(8)
    frames = torch.from_numpy(st["frames"][:n]).cuda()
    out = torch.full((n, 24), FILL, dtype=torch.uint8, device="cuda")
    states = torch.zeros((2, nb), dtype=torch.uint8, device="cuda")
    results = torch.zeros((n, RESULT_BYTES), dtype=torch.uint8, device="cuda")
    for k in range(n):
        pctx.packet_fec_erasures_dev([dabgpu.PacketFecErasureEntry(frames[k].data_ptr(), 24, 8, 0, out[k].data_ptr(), 24, states[k & 1].data_ptr() if k else None,
                                                                   states[(k & 1) ^ 1].data_ptr(), results[k].data_ptr())], 1)
    pctx.sync()
    whole = run_cut(HostMemory, dict(st, frames=st["frames"][:n]), [])
    res = results.cpu().numpy().view(dabgpu.PACKET_FEC_ERASURE_RESULT_DTYPE).reshape(n)
    assert (out.cpu().numpy() == whole[0]).all() and E.total([res[k:k + 1] for k in range(n)]) == whole[1]
    assert states[n & 1].cpu().numpy().tobytes() == whole[2] and whole[1]["frames"] == 1 and whole[1]["rows_erasure_corrected"] == 12
    assert int(res[102]["frames"]) == 1 and int(res[102]["rows_erasure_corrected"]) == 12 and int(res[102]["frames_with_suspects"]) == 1
    assert [k for k in range(103) if int(res[k]["slots_suspect"])] == [2, 30, 47, 70, 93]


@pytest.mark.gpu
def test_gpu_refused_calls_leave_every_output_alone(pctx, limit):
    specs, n = refusal_specs()
    for m in P.BAD_ENTRIES:
        call(DeviceMemory(pctx), specs, n, mutate=m, refused=ARG)
    pctx.packet_fec_erasures_dev([], 4)                               # nothing to do is not an error
    got = call(DeviceMemory(pctx), specs, n)
    host = call(HostMemory(), specs, n)
    assert all(same(g, h) for g, h in zip(got, host))
