"""RS(204,188) correction of packet-mode FEC frames (dabgpu_packet_fec_dev, dabgpu_packet_fec_host; the contract:
include/dabgpu_packet_fec.h) against tests/packet_fec_reference.py, a restatement of EN 300 401 clause 5.3.5 that decodes by
Euclid's algorithm without tables and verifies every correction by definition.  Each stream below is about one clause; its
`counts` are asserted on the REFERENCE's result before the code under test is held to it.  See tests/README_packet_fec.md."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import packet_fec_reference as F
import packet_reference as R
import test_packet as T
from conftest import ROOT
from test_device_asm import CSRC, kernel_metadata

ARG, CAPACITY = -1, -6
FILL, GAP = 0xA7, 64
ADDR = T.ADDR
RATES = (8, 24, 40, 256, 512)


# ------------------------------------------------------------------------------------------------ building streams
def random_packets(rng, n_slots, address=ADDR):
    """packets of 1 .. 4 slots with random useful bytes, n_slots in all"""
    out, k = [], 0
    while n_slots > 0:
        L = min(int(rng.integers(1, 5)), n_slots)
        out.append(synth.packet(address, bytes(rng.integers(0, 256, 24 * L - 5, dtype=np.uint8)), L, ci=k, first=True, last=True))
        n_slots -= L
        k += 1
    return out


def clean_frames(bitrate, seed, tables=3):
    """just long enough for `tables` FEC frames to come out: their slots, then the delay"""
    S = bitrate // 8
    rng = np.random.default_rng(seed)
    pk = [synth.packet(ADDR, bytes(rng.integers(0, 256, 19, dtype=np.uint8)), 1, ci=k) for k in range(94 * tables)] if S < 4 else \
        random_packets(rng, 80 * tables)
    n = -(-103 * tables // S)
    fr = np.concatenate([synth.packet_fec_frames(bitrate, [pk], n_frames=n)[:n], synth.packet_frames(bitrate, [], n_frames=F.delay(bitrate))])
    assert fr.shape == (n + F.delay(bitrate), 3 * bitrate)
    return fr


def at(frames, table, row, c):
    """(flat index of) byte c of row `row`'s codeword in FEC frame `table` of a stream whose first table begins at slot 0"""
    if c < 188:
        b = 12 * c + row
        return (103 * table + b // 24) * 24 + b % 24
    p = 12 * (c - 188) + row
    return (103 * table + 94 + p // 22) * 24 + 2 + p % 22


def hit(frames, table, row, positions, values=None, rng=None):
    """errors in one row: values XORed in (non-zero: random from rng, or as given)"""
    flat = frames.reshape(-1)
    for k, c in enumerate(positions):
        v = values[k] if values is not None else int(rng.integers(1, 256))
        flat[at(frames, table, row, c)] ^= v


def wipe(frames, slot, rng):
    """a whole 24-byte slot overwritten (never by something that reads as a mark)"""
    flat = frames.reshape(-1, 24)
    new = rng.integers(0, 256, 24, dtype=np.uint8)
    new[0] |= 0x40
    flat[slot] = new


def stream(bitrate, sent, received, **counts):
    return dict(bitrate=bitrate, sent=sent, frames=received, counts=counts)


def _streams():
    S = {}
    rng = np.random.default_rng(2024)

    # rows with errors: 0, 1, 7 and 8 of them; at the ends of the data and of the parity; in the parity alone; two of one value
    sent = clean_frames(32, 1)
    fr = sent.copy()
    hit(fr, 0, 1, [17], rng=rng)
    hit(fr, 0, 2, [3, 30, 60, 90, 120, 150, 180], rng=rng)
    hit(fr, 0, 3, [5, 6, 7, 99, 100, 170, 186, 187], rng=rng)
    hit(fr, 0, 4, [0, 187, 188, 203], rng=rng)
    hit(fr, 0, 5, [190, 200], rng=rng)
    hit(fr, 0, 6, [10, 20], values=[0x5A, 0x5A])
    hit(fr, 1, 11, [0, 1, 2, 3, 199, 201, 202, 203], rng=rng)
    S["rows"] = stream(32, sent, fr, frames=3, frames_cut=0, frames_overlapping=0, marks=27, rows_clean=29, rows_corrected=7, rows_uncorrectable=0,
                       bytes_corrected=1 + 7 + 8 + 2 + 0 + 2 + 4, parity_bytes_corrected=2 + 2 + 4)

    # whole packets overwritten: four are 8 errors a row, five are 10
    sent = clean_frames(32, 2)
    fr = sent.copy()
    for s in (3, 20, 50, 93):
        wipe(fr, 103 * 0 + s, rng)
    for s in (0, 11, 40, 41, 77):
        wipe(fr, 103 * 1 + s, rng)
    S["packets"] = stream(32, sent, fr, frames=3, marks=27, rows_clean=12, rows_corrected=12, rows_uncorrectable=12)

    # beyond the bound: 9 .. 12 random errors in each of 2004 rows
    sent = clean_frames(512, 3, tables=167)
    fr = sent.copy()
    for t in range(167):
        for r in range(12):
            n = 9 + (12 * t + r) % 4
            hit(fr, t, r, rng.choice(204, n, replace=False), rng=rng)
    S["beyond"] = stream(512, sent, fr, frames=167, marks=9 * 167, rows_clean=0)

    # marks
    sent = clean_frames(32, 4)
    fr = sent.copy()
    flat = fr.reshape(-1, 24)
    flat[103 + 94 + 2, 1] ^= 0x10                                     # two damaged FEC headers: still found
    flat[103 + 94 + 7, 0] ^= 0x80
    wipe(fr, 103 + 9, rng)
    S["two bad marks"] = stream(32, sent, fr, frames=3, marks=25, rows_clean=24, rows_corrected=12, rows_uncorrectable=0)
    fr = sent.copy()
    flat = fr.reshape(-1, 24)
    for i in (0, 4, 8):
        flat[103 + 94 + i, 1] ^= 0x01                                 # three: the frame is not found, its damaged packet stays
    wipe(fr, 103 + 9, rng)
    S["three bad marks"] = stream(32, sent, fr, frames=2, marks=24, rows_clean=24, rows_corrected=0, rows_uncorrectable=0)
    fr = sent.copy()
    flat = fr.reshape(-1, 24)
    flat[103 + 94 + 5, 0] = (flat[103 + 94 + 5, 0] & 0xC3) | (9 << 2)    # a counter of 9 is no mark
    flat[2 * 103 + 94 + 0, 0] = (flat[2 * 103 + 94, 0] & 0xC3) | (1 << 2)  # a mark in the wrong place counts as one, not as a hit
    S["counter 9"] = stream(32, sent, fr, frames=3, marks=26, rows_clean=36, rows_corrected=0, rows_uncorrectable=0)
    fr = sent.copy()
    flat = fr.reshape(-1, 24)
    for i in range(9):                                                # the nine marks again, 20 slots into the second table
        flat[103 + 20 + i] = flat[94 + i]
    S["overlap"] = stream(32, sent, fr, frames=3, frames_overlapping=1, marks=36, rows_clean=24, rows_uncorrectable=12)
    whole = clean_frames(32, 5, tables=4)
    cut = whole[7:].copy()                                            # begins 28 slots into the first table
    wipe(cut, 103 - 28 + 5, rng)
    S["mid-frame"] = stream(32, whole[7:], cut, frames=3, frames_cut=1, marks=36, rows_clean=24, rows_corrected=12, rows_uncorrectable=0)
    plain = synth.packet_frames(32, [random_packets(np.random.default_rng(6), 120)], n_frames=60)
    S["no fec"] = stream(32, plain, plain.copy(), frames=0, frames_cut=0, frames_overlapping=0, marks=0, rows_clean=0, rows_corrected=0, rows_uncorrectable=0)

    # bit rates: S = 1, 3, 5, 32, 64 and D = 102, 34, 21, 4, 2; one damaged packet in every FEC frame
    for rate in RATES:
        sent = clean_frames(rate, 10 + rate)
        fr = sent.copy()
        for t in range(3):
            wipe(fr, 103 * t + 13 + 31 * t, rng)
        S["rate %d" % rate] = stream(rate, sent, fr, frames=3, marks=27, rows_clean=0, rows_corrected=36, rows_uncorrectable=0)
    return S


STREAM_NAMES = ["rows", "packets", "beyond", "two bad marks", "three bad marks", "counter 9", "overlap", "mid-frame", "no fec"] + ["rate %d" % r for r in RATES]
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
        out, counts = F.Receiver(st["bitrate"]).call(st["frames"])
        out.setflags(write=False)
        _WANTS[name] = (out, counts)
    return _WANTS[name]


# ------------------------------------------------------------------------------------------------ one call, on any memory
class HostMemory:
    def load(self, img):
        raw = np.empty(img.size + 256, np.uint8)
        off = -raw.ctypes.data % 256
        self.buf = raw[off:off + img.size]
        self.buf[:] = img
        return self.buf.ctypes.data

    def run(self, entries, n_cifs):
        dabgpu.packet_fec_host(entries, n_cifs)

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
        self.ctx.packet_fec_dev(entries, n_cifs)
        self.ctx.sync()

    def read(self):
        self.ctx.sync()
        return self.t.cpu().numpy()


def call(mem, specs, n_cifs, mutate=None, refused=None):
    """One call on buffers laid out in one allocation, every region between sentinel bytes.  specs: dicts {bitrate, frames (at
    least n_cifs rows), state (bytes or None = NULL), stride (in_stride), out_stride, in_off, out_off (the frames begin that
    many bytes off their 256-byte boundary)}.  After the call nothing but the n_cifs output frames, state-out and the result
    may have changed (nothing at all for a refused call).  -> per entry dict(out [n_cifs][3 R], result, state)"""
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
                        sin=take(nb) if sp.get("state") is not None else None, sout=take(nb), result=take(48)))
    img = np.full(size + GAP, FILL, np.uint8)
    for sp, L in zip(specs, lay):
        for k in range(n_cifs):
            img[L["frames"] + k * L["stride"]:L["frames"] + k * L["stride"] + L["fb"]] = sp["frames"][k]
        if L["sin"] is not None:
            img[L["sin"]:L["sin"] + L["nb"]] = np.frombuffer(bytes(sp["state"]), np.uint8)
    base = mem.load(img)
    assert base % 256 == 0
    entries = [dabgpu.PacketFecEntry(base + L["frames"], L["stride"], sp["bitrate"], 0, base + L["out"], L["ostride"],
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
        untouched[L["result"]:L["result"] + 48] = False
        rows = np.zeros((n_cifs, L["fb"]), np.uint8)
        for k in range(n_cifs):
            a = L["out"] + k * L["ostride"]
            untouched[a:a + L["fb"]] = False
            rows[k] = after[a:a + L["fb"]]
        out.append(dict(out=rows, result=after[L["result"]:L["result"] + 48].copy().view(dabgpu.PACKET_FEC_RESULT_DTYPE),
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
    return np.concatenate(outs), F.total(results), state


def counts_of(rec):
    return {k: int(rec[k][0]) for k in F.COUNTERS}


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_records_and_sizes(built, tmp_path):
    L = dabgpu.lib()
    for name in ("dabgpu_packet_fec_state_bytes", "dabgpu_packet_fec_delay", "dabgpu_packet_fec_dev", "dabgpu_packet_fec_host"):
        assert name in dabgpu.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.dabgpu_abi_version() == 6 == dabgpu.ABI_VERSION
    assert dabgpu.PACKET_FEC_RESULT_DTYPE.itemsize == 48 == F.RESULT_DTYPE.itemsize and dabgpu.PACKET_FEC_RESULT_DTYPE.names == F.RESULT_DTYPE.names
    assert hasattr(dabgpu.Context, "packet_fec_dev")
    for rate in range(8, 520, 8):
        S = rate // 8
        D = -(-102 // S)
        assert dabgpu.packet_fec_delay(rate) == D == F.delay(rate)
        nb = dabgpu.packet_fec_state_bytes(rate)
        assert nb % 16 == 0 and 24 * S * D < nb < 4100, (rate, nb)
    assert (dabgpu.packet_fec_delay(8), dabgpu.packet_fec_delay(512)) == (102, 2)
    for bad in (0, 4, 12, 520, -8):
        assert L.dabgpu_packet_fec_state_bytes(bad) == 0 and L.dabgpu_packet_fec_delay(bad) == -1
        with pytest.raises(ValueError):
            dabgpu.packet_fec_state_bytes(bad)
    # the binding's structure and the record against the header, as the C compiler lays them out
    lines, want = ['#include <stdio.h>', '#include <stddef.h>', '#include "dabgpu.h"', 'int main(void) {'], []
    lines.append('  printf(" %zu", sizeof(dabgpu_packet_fec_entry));')
    lines += ['  printf(" %%zu", offsetof(dabgpu_packet_fec_entry, %s));' % f for f, _ in dabgpu.PacketFecEntry._fields_]
    want += [C.sizeof(dabgpu.PacketFecEntry)] + [getattr(dabgpu.PacketFecEntry, f).offset for f, _ in dabgpu.PacketFecEntry._fields_]
    dt = dabgpu.PACKET_FEC_RESULT_DTYPE
    lines.append('  printf(" %zu", sizeof(dabgpu_packet_fec_result));')
    lines += ['  printf(" %%zu", offsetof(dabgpu_packet_fec_result, %s));' % f for f in dt.names]
    want += [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ['  return 0; }']) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == want


def test_transmit_side_is_what_the_contract_says():
    """rs204_parity makes codewords of the reference's code; fec_frame lays the tables out column by column; packet_fec_frames
    keeps packets inside logical frames and tables; the padding packet of the delay is synth's"""
    rng = np.random.default_rng(0)
    rows = rng.integers(0, 256, (5, 188), dtype=np.uint8)
    cw = np.concatenate([rows, np.stack([synth.rs204_parity(r) for r in rows])], axis=1)
    assert cw.shape == (5, 204) and not F.syndromes(cw).any()
    assert F.syndromes(cw ^ np.eye(204, dtype=np.uint8)[:5]).all(axis=1).all()
    assert bytes(F.PADDING_PACKET) == synth.packet(0, b"", 1, fill=0) and F.PADDING_PACKET[:3] == bytes([0x0C, 0, 0])
    data = bytes(rng.integers(0, 256, 2256, dtype=np.uint8))
    ff = synth.fec_frame(data)
    assert len(ff) == 103 * 24 and ff[:2256] == data
    p = b"".join(ff[2256 + 24 * c + 2:2256 + 24 * c + 24] for c in range(9))
    assert [F.mark(ff[2256 + 24 * c:]) for c in range(9)] == list(range(9)) and p[192:] == bytes(6)
    table = np.array([[data[12 * c + r] for c in range(188)] + [p[12 * j + r] for j in range(16)] for r in range(12)], np.uint8)
    assert not F.syndromes(table).any()
    for rate in (8, 40, 72, 512):
        S = rate // 8
        pk = random_packets(rng, 300) if S >= 4 else [synth.packet(3, b"x", 1, ci=k) for k in range(200)]
        fr = synth.packet_fec_frames(rate, [pk[:len(pk) // 2], pk[len(pk) // 2:]], n_frames=3)
        flat = fr.reshape(-1, 24)
        n_tables = len(flat) // 103
        assert n_tables >= 1 and fr.shape[1] == 3 * rate
        for t in range(n_tables):
            assert flat[103 * t:103 * t + 103].tobytes() == synth.fec_frame(flat[103 * t:103 * t + 94].tobytes())
        # every packet lies inside its logical frame and inside its table: the scan of each frame meets nothing bad
        rx = R.Receiver(1024, ADDR, 1)
        _slides, counts = rx.call(fr, rate, 1, 1024)
        assert int(counts["slots_bad"][0]) == 0 and int(counts["packets_fec"][0]) == 9 * n_tables
        for t in range(n_tables):
            k = 103 * t
            while k < 103 * t + 94:
                k += (int(flat[k, 0]) >> 6) + 1
            assert k == 103 * t + 94, "a packet straddles the table"


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_host_equals_the_reference(built, name):
    """each stream in one call: the stream's own expectations on the REFERENCE's result first, then the host twin against it,
    byte for byte; the first D output frames are padding packets; what was corrected is what was sent"""
    st = streams()[name]
    want, wc = wanted(name)
    ref = counts_of(wc)
    for key, v in st["counts"].items():
        assert ref[key] == v, (name, key, ref)
    D, S = F.delay(st["bitrate"]), st["bitrate"] // 8
    assert ref["cifs"] == len(st["frames"]) and ref["slots"] == S * len(st["frames"])
    assert ref["rows_clean"] + ref["rows_corrected"] + ref["rows_uncorrectable"] == 12 * ref["frames"]
    assert (want[:D] == np.frombuffer(synth.packet(0, b"", 1, fill=0) * S, np.uint8)).all()
    got = call(HostMemory(), [dict(bitrate=st["bitrate"], frames=st["frames"])], len(st["frames"]))[0]
    assert counts_of(got["result"]) == ref and got["result"].tobytes() == wc.tobytes(), (name, got["result"], wc)
    assert (got["out"] == want).all(), name
    if name in ("rows", "two bad marks", "counter 9", "mid-frame", "no fec") or name.startswith("rate"):
        data = np.ones(len(st["sent"]) * S, bool)
        if name != "no fec":
            data[(np.arange(len(data)) + (28 if name == "mid-frame" else 0)) % 103 >= 94] = False
        n = len(st["frames"]) - D
        assert (want[D:].reshape(-1, 24)[data[:n * S]] == st["sent"][:n].reshape(-1, 24)[data[:n * S]]).all(), "the data as sent"
    if name == "three bad marks":
        raw, sent = st["frames"].reshape(-1, 24), st["sent"].reshape(-1, 24)
        assert (want[D:].reshape(-1, 24)[103:206] == raw[103:206]).all() and (raw[103 + 9] != sent[103 + 9]).any()
    if name == "packets":
        raw, sent, out = st["frames"].reshape(-1, 24), st["sent"].reshape(-1, 24), want[D:].reshape(-1, 24)
        assert (out[:94] == sent[:94]).all() and (out[103:206] == raw[103:206]).all() and ref["bytes_corrected"] > 4 * 24 - 8


def test_rows_beyond_the_bound_are_decided_by_the_reference(built):
    """2004 rows with 9 .. 12 errors: the reference decides each -- unchanged, or (a share near 1 / 8! of them) taken for a
    codeword within 8 of something else -- and the twin agreed byte for byte (test_host_equals_the_reference).  The reference's
    own result holds at least one uncorrectable row; none is miscorrected."""
    _want, wc = wanted("beyond")
    ref = counts_of(wc)
    print("rows beyond the bound: %d uncorrectable, %d miscorrected of %d" % (ref["rows_uncorrectable"], ref["rows_corrected"], 12 * ref["frames"]))
    assert ref["frames"] == 167 and ref["rows_uncorrectable"] >= 1
    assert ref["rows_corrected"] == 0 and ref["rows_uncorrectable"] == 2004 and ref["bytes_corrected"] == 0


def test_reference_corrects_what_the_definition_says_it_must():
    """the reference on its own: every pattern of 1 .. 8 errors in a codeword comes back; a row is only ever changed into a
    codeword at most 8 positions away"""
    rng = np.random.default_rng(9)
    rows = rng.integers(0, 256, (40, 188), dtype=np.uint8)
    cw = np.concatenate([rows, np.stack([synth.rs204_parity(r) for r in rows])], axis=1)
    bad = cw.copy()
    for i in range(40):
        for c in rng.choice(204, 1 + i % 8, replace=False):
            bad[i, c] ^= rng.integers(1, 256)
    fixed, verdicts = F.correct_rows(bad)
    assert (fixed == cw).all() and verdicts == [1 + i % 8 for i in range(40)]
    assert F.correct_rows(cw)[1] == [0] * 40


CUT_NAMES = [n for n in STREAM_NAMES if n != "beyond"]


@pytest.mark.parametrize("name", CUT_NAMES)
def test_cut_into_two_and_three_calls_at_every_frame_boundary(built, name):
    """the result of a stream does not depend on where it is cut: two calls at every frame boundary, three calls at every pair of
    neighbouring boundaries (the middle call is one frame: fewer than D), and calls of no frame at all: output, summed counters
    and the last state record equal the uncut run's"""
    st = streams()[name]
    n = len(st["frames"])
    whole = run_cut(HostMemory, st, [])
    assert (whole[0] == wanted(name)[0]).all()
    for k in range(0, n + 1):
        got = run_cut(HostMemory, st, [k])
        assert (got[0] == whole[0]).all() and got[1] == whole[1] and got[2] == whole[2], (name, k)
    for k in range(0, n):
        got = run_cut(HostMemory, st, [k, k + 1])
        assert (got[0] == whole[0]).all() and got[1] == whole[1] and got[2] == whole[2], (name, k)
    got = run_cut(HostMemory, st, [n // 3, n // 3, n // 2, n // 2, n // 2])
    assert (got[0] == whole[0]).all() and got[1] == whole[1] and got[2] == whole[2]


def test_the_long_stream_cut_into_calls(built):
    """the stream of 167 FEC frames (D = 2): two calls at every 7th boundary and around the first frames, three at the same"""
    st = streams()["beyond"]
    n = len(st["frames"])
    whole = run_cut(HostMemory, st, [])
    assert (whole[0] == wanted("beyond")[0]).all()
    for k in list(range(0, 6)) + list(range(6, n + 1, 7)):
        for cuts in ([k], [k, min(k + 1, n)]):
            got = run_cut(HostMemory, st, cuts)
            assert (got[0] == whole[0]).all() and got[1] == whole[1] and got[2] == whole[2], cuts


def test_foreign_and_all_zero_state_records_are_a_fresh_start(built):
    st = streams()["rate 40"]
    nb = dabgpu.packet_fec_state_bytes(40)
    whole = run_cut(HostMemory, st, [])
    for state in (bytes(nb), bytes(np.random.default_rng(5).integers(0, 256, nb, dtype=np.uint8)), bytes([0xFF]) * nb):
        got = run_cut(HostMemory, st, [], first_state=state)
        assert (got[0] == whole[0]).all() and got[1] == whole[1] and got[2] == whole[2]
    # a record of another bit rate is none of this one's: 32 and 40 kbit/s have records of one size
    other = run_cut(HostMemory, streams()["rows"], [])[2]
    got = run_cut(HostMemory, st, [], first_state=(other + bytes(nb))[:nb])
    assert (got[0] == whole[0]).all() and got[1] == whole[1] and got[2] == whole[2]
    # a record of this bit rate is not: the stream goes on behind it, and the first output frames are the carried ones (the
    # last D frames of the run before lie behind its last FEC frame: they are as received)
    D = F.delay(40)
    again = run_cut(HostMemory, st, [], first_state=whole[2])
    assert (again[0][:D] == st["frames"][-D:]).all() and (again[0][D:] == whole[0][D:]).all()
    assert again[1] == whole[1] and again[2] != whole[2]


# ---- refusals
def spoil(field, value):
    def m(entries):
        setattr(entries[-1], field, value(entries[-1]) if callable(value) else value)
    return m


BAD_ENTRIES = [spoil("bitrate_kbps", 0), spoil("bitrate_kbps", 12), spoil("bitrate_kbps", 520), spoil("bitrate_kbps", -8),
               spoil("in_stride", lambda e: 3 * e.bitrate_kbps - 1), spoil("out_stride", lambda e: 3 * e.bitrate_kbps - 1), spoil("out_stride", 0),
               spoil("d_in", None), spoil("d_out", None), spoil("d_state_out", None), spoil("d_result", None),
               spoil("d_state_in", lambda e: e.d_state_in + 8), spoil("d_state_out", lambda e: e.d_state_out + 4), spoil("d_result", lambda e: e.d_result + 2),
               spoil("d_state_in", lambda e: e.d_state_out), spoil("d_state_in", lambda e: e.d_state_out + 16),
               spoil("d_state_in", lambda e: e.d_state_out - 16), spoil("d_out", lambda e: e.d_in), spoil("d_out", lambda e: e.d_in + 1),
               spoil("d_out", lambda e: e.d_in + 5 * e.in_stride + 3 * e.bitrate_kbps - 1), spoil("d_out", lambda e: e.d_in - 5 * e.out_stride - 3 * e.bitrate_kbps + 1)]


def refusal_specs():
    st = streams()["rate 40"]
    nb = dabgpu.packet_fec_state_bytes(40)
    return [dict(bitrate=40, frames=st["frames"], state=bytes(nb), stride=128, out_stride=130, in_off=3, out_off=7) for _ in range(3)], 6


def test_refusals_that_need_no_device(built):
    specs, n = refusal_specs()
    for m in BAD_ENTRIES:
        call(HostMemory(), specs, n, mutate=m, refused=ARG)
    L = dabgpu.lib()
    e = (dabgpu.PacketFecEntry * 1)()
    assert L.dabgpu_packet_fec_host(None, 1, 1) == ARG and L.dabgpu_packet_fec_host(e, -1, 1) == ARG and L.dabgpu_packet_fec_host(e, 1, -1) == ARG
    assert L.dabgpu_packet_fec_host(e, 1, (1 << 24) + 1) == ARG and L.dabgpu_packet_fec_dev(None, e, 1, 1, None) == ARG
    dabgpu.packet_fec_host([], 3)                                      # nothing to do is not an error
    # d_in and d_out may both be NULL when there is no frame; the state record still moves on
    got = call(HostMemory(), specs, 0, mutate=lambda es: [setattr(x, "d_in", None) or setattr(x, "d_out", None) for x in es])
    assert all(counts_of(g["result"]) == dict.fromkeys(F.COUNTERS, 0) for g in got)


# ---- device code, sanitizers
def test_new_kernels_neither_spill_nor_use_scratch(built, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the device assembly cannot be checked")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "packet_fec_kernels.hip" in mk and "dabgpu_packet_fec_api.hip" in mk and "dabgpu_packet_fec.h" in mk
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    out = tmp_path / "packet_fec_kernels.s"
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "packet_fec_kernels.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    md = kernel_metadata(out.read_text())
    # the file holds both calls' kernels: this call's four, each once, and the erasure call's four, and no others
    assert all(sum(k in name for name in md) == 1 for k in ("packet_fec_move_kernel", "packet_fec_accept_kernel",
                                                            "packet_fec_correct_kernel", "packet_fec_tally_kernel"))
    assert len(md) == 8 and all(sum(k in name for name in md) == 1 for k in ("packet_fec_erasure_move_kernel", "packet_fec_erasure_accept_kernel",
                                                                            "packet_fec_erasure_correct_kernel", "packet_fec_erasure_tally_kernel"))
    for k, v in md.items():
        print("%s: vgprs %s, sgprs %s, LDS %s bytes" % (k, v.get("vgpr_count"), v.get("sgpr_count"), v.get("group_segment_fixed_size")))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)


def test_fec_fuzz_under_sanitizers(tmp_path):
    """tests/packet_fec_fuzz.cpp: random frames, random marks and random state records through the header's host path, every
    buffer a heap block of exactly its size; a stand-alone program built with the host compiler under AddressSanitizer and UBSan
    and run as a child process"""
    exe = str(tmp_path / "packet_fec_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "packet_fec_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "calls=3000" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = dict(kv.split("=") for kv in r.stdout.split())
    print(r.stdout)
    for key in ("frames", "cut", "overlapping", "clean", "corrected", "uncorrectable", "fresh", "carried", "empty"):
        assert int(got[key]) > 0, (key, r.stdout)


# ---- the chain: FEC in front of the slides call
CHAIN_OBJECT = T.obj(0x611, 500, 41, b"fec.png", 200)


def chain_frames():
    """32 kbit/s: one slide, carried once, in one-slot packets, behind it padding; in every FEC frame one packet of it wiped"""
    pk = synth.packetise(CHAIN_OBJECT[2], ADDR, sizes=(1,))
    sent = np.concatenate([synth.packet_fec_frames(32, [pk], n_frames=52)[:52], synth.packet_frames(32, [], n_frames=F.delay(32))])
    assert len(pk) < 94
    raw = sent.copy()
    rng = np.random.default_rng(8)
    for t in range(2):
        wipe(raw, 103 * t + 11, rng)
    return sent, raw


def slides_host(frames, fec=1):
    sp = dict(bitrate=32, frames=frames, address=ADDR, fec=fec, state=None, body_capacity=1024, max_slides=2)
    return T.call(T.HostMemory(), [sp], len(frames))[0]


def test_chain_fec_then_slides_delivers_what_the_raw_frames_lose(built):
    _sent, raw = chain_frames()
    header, body = CHAIN_OBJECT[0], CHAIN_OBJECT[1]
    lost, lc = R.Receiver(1024, ADDR, 1).call(raw, 32, 2, 1024)       # the REFERENCE on the raw frames: the slide is lost
    assert lost == [] and int(lc["slots_bad"][0]) >= 1 and int(lc["continuity_breaks"][0]) >= 1
    fixed = call(HostMemory(), [dict(bitrate=32, frames=raw)], len(raw))[0]
    assert counts_of(fixed["result"])["rows_corrected"] == 24 and counts_of(fixed["result"])["frames"] == 2
    got = slides_host(fixed["out"])
    assert T.strip(got["slides"]) == [(0x611, 2, 1, header, body)]
    res = got["result"]
    assert int(res["slots_bad"][0]) == 0 and int(res["packets_fec"][0]) == 9 * 2 and int(res["packets_padding"][0]) >= 4 * F.delay(32)
    # `superframe` of the slide counts delayed frames
    want, _wc = R.Receiver(1024, ADDR, 1).call(_sent, 32, 2, 1024)
    assert int(got["slides"][0][0]["superframe"][0]) == int(want[0][0]["superframe"][0]) + F.delay(32)


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


def all_specs(n_cifs):
    """every stream as one entry of one table, frames of 0xFF behind the shorter ones: in_stride and out_stride beyond 3 R and
    frames off their 16-byte and 4-byte boundaries by turns"""
    specs = []
    for e, name in enumerate(STREAM_NAMES):
        st = streams()[name]
        fr = st["frames"][:n_cifs]
        if len(fr) < n_cifs:
            fr = np.concatenate([fr, np.full((n_cifs - len(fr), fr.shape[1]), 0xFF, np.uint8)])
        specs.append(dict(bitrate=st["bitrate"], frames=fr, stride=3 * st["bitrate"] + [0, 2, 16, 5][e % 4], out_stride=3 * st["bitrate"] + [0, 16, 3, 4][(e // 2) % 4],
                          in_off=[0, 8, 4, 1, 13][e % 5], out_off=[0, 4, 0, 7, 16][(e + 1) % 5]))
    return specs


def same(g, h):
    return g["result"].tobytes() == h["result"].tobytes() and (g["out"] == h["out"]).all() and g["state"].tobytes() == h["state"].tobytes()


@pytest.mark.gpu
def test_gpu_every_stream_in_one_call(pctx):
    """all streams in ONE call of 411 logical frames (rows of 0xFF behind the shorter streams): bit rates from 8 to 512,
    strides beyond 3 R, d_in and d_out off 16 and off 4 bytes: output, counters and state record equal the host call's byte
    for byte, and the reference's where the stream lies"""
    n = max(len(streams()[name]["frames"]) for name in STREAM_NAMES)
    assert n == 411
    specs = all_specs(n)
    got = call(DeviceMemory(pctx), specs, n)
    host = call(HostMemory(), specs, n)
    for name, g, h in zip(STREAM_NAMES, got, host):
        assert same(g, h), (name, g["result"], h["result"])
        want, wc = wanted(name)
        assert (g["out"][:len(want)] == want).all(), name
        ref, mine = counts_of(wc), counts_of(g["result"])
        assert {k: mine[k] for k in F.COUNTERS[2:]} == {k: ref[k] for k in F.COUNTERS[2:]}, name
    assert sum(counts_of(g["result"])["rows_corrected"] for g in got) >= 200 and sum(counts_of(g["result"])["rows_uncorrectable"] for g in got) >= 2000


@pytest.mark.gpu
@pytest.mark.parametrize("n_cifs", [0, 1, 7])
def test_gpu_short_calls(pctx, n_cifs):
    """calls of 0, 1 and 7 logical frames, every entry, from a fresh start and from the state the host left after 30 frames"""
    specs = all_specs(n_cifs)
    got = call(DeviceMemory(pctx), specs, n_cifs)
    host = call(HostMemory(), specs, n_cifs)
    for name, g, h in zip(STREAM_NAMES, got, host):
        assert same(g, h), name
    longer = all_specs(30 + n_cifs)
    first = call(HostMemory(), [dict(sp, frames=sp["frames"][:30]) for sp in longer], 30)
    later = [dict(sp, frames=sp["frames"][30:], state=f["state"].tobytes()) for sp, f in zip(longer, first)]
    got = call(DeviceMemory(pctx), later, n_cifs)
    host = call(HostMemory(), later, n_cifs)
    for name, g, h in zip(STREAM_NAMES, got, host):
        assert same(g, h), name


@pytest.mark.gpu
def test_gpu_130_entries_in_one_table(pctx):
    """130 entries: the thirteen streams of 32 kbit/s and below 512, ten times over, 110 frames each, outputs of their own"""
    names = [n for n in STREAM_NAMES if n != "beyond"]
    assert len(names) == 13
    base = {sp_name: sp for sp_name, sp in zip(STREAM_NAMES, all_specs(110))}
    specs = [dict(base[n], out_stride=3 * base[n]["bitrate"] + 3 * (k % 2)) for k in range(10) for n in names]
    got = call(DeviceMemory(pctx), specs, 110)
    host = call(HostMemory(), specs[:13], 110)
    for k, g in enumerate(got):
        assert same(g, host[k % 13]), (k, names[k % 13])
    assert sum(counts_of(g["result"])["frames"] for g in got) >= 130


@pytest.mark.gpu
def test_gpu_two_calls_back_to_back_with_the_state_on_the_device(pctx):
    """every stream in two calls enqueued one behind the other, nothing waiting in between, cut in the middle of the stream where
    an FEC frame straddles the calls: the state record of the first is the second's input: output, summed counters and the
    last state equal the uncut host run's"""
    import torch
    bufs = {}
    for name in STREAM_NAMES:
        st = streams()[name]
        n, nb, fb = len(st["frames"]), dabgpu.packet_fec_state_bytes(st["bitrate"]), 3 * st["bitrate"]
        cut = 2 * n // 5
        assert (cut * (st["bitrate"] // 8)) % 103 not in (0, 102)
        bufs[name] = dict(frames=torch.from_numpy(st["frames"]).cuda(), out=torch.full((n, fb), FILL, dtype=torch.uint8, device="cuda"), cut=cut,
                          states=torch.zeros((2, nb), dtype=torch.uint8, device="cuda"), results=torch.zeros((2, 48), dtype=torch.uint8, device="cuda"))
    for k in range(2):
        for name in STREAM_NAMES:
            st, b = streams()[name], bufs[name]
            a, n_cifs = (b["cut"], len(st["frames"]) - b["cut"]) if k else (0, b["cut"])
            pctx.packet_fec_dev([dabgpu.PacketFecEntry(b["frames"][a].data_ptr(), 3 * st["bitrate"], st["bitrate"], 0, b["out"][a].data_ptr(), 3 * st["bitrate"],
                                                       b["states"][0].data_ptr() if k else None, b["states"][k].data_ptr(), b["results"][k].data_ptr())], n_cifs)
    pctx.sync()
    for name in STREAM_NAMES:
        b, st = bufs[name], streams()[name]
        whole = run_cut(HostMemory, st, [])
        res = b["results"].cpu().numpy().view(dabgpu.PACKET_FEC_RESULT_DTYPE).reshape(2)
        assert (b["out"].cpu().numpy() == whole[0]).all(), name
        assert F.total([res[k:k + 1] for k in range(2)]) == whole[1], name
        assert b["states"][1].cpu().numpy().tobytes() == whole[2], name


@pytest.mark.gpu
def test_gpu_single_frame_calls_across_an_fec_frame(pctx):
    """8 kbit/s, S = 1: 140 calls of one frame each (one slot), across the first FEC frame's end and into the second, the state
    ping-ponging on the device, nothing waiting in between"""
    import torch
    st = streams()["rate 8"]
    n, nb = 140, dabgpu.packet_fec_state_bytes(8)
    frames = torch.from_numpy(st["frames"][:n]).cuda()
    out = torch.full((n, 24), FILL, dtype=torch.uint8, device="cuda")
    states = torch.zeros((2, nb), dtype=torch.uint8, device="cuda")
    results = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
    for k in range(n):
        pctx.packet_fec_dev([dabgpu.PacketFecEntry(frames[k].data_ptr(), 24, 8, 0, out[k].data_ptr(), 24, states[k & 1].data_ptr() if k else None,
                                                   states[(k & 1) ^ 1].data_ptr(), results[k].data_ptr())], 1)
    pctx.sync()
    whole = run_cut(HostMemory, dict(st, frames=st["frames"][:n]), [])
    res = results.cpu().numpy().view(dabgpu.PACKET_FEC_RESULT_DTYPE).reshape(n)
    assert (out.cpu().numpy() == whole[0]).all() and F.total([res[k:k + 1] for k in range(n)]) == whole[1]
    assert states[n & 1].cpu().numpy().tobytes() == whole[2] and whole[1]["frames"] == 1 and whole[1]["rows_corrected"] == 12
    assert int(res[102]["frames"]) == 1 and int(res[102]["rows_corrected"]) == 12


@pytest.mark.gpu
def test_gpu_refused_calls_leave_every_output_alone(pctx):
    specs, n = refusal_specs()
    for m in BAD_ENTRIES:
        call(DeviceMemory(pctx), specs, n, mutate=m, refused=ARG)
    pctx.packet_fec_dev([], 4)                                        # nothing to do is not an error
    got = call(DeviceMemory(pctx), specs, n)
    host = call(HostMemory(), specs, n)
    assert all(same(g, h) for g, h in zip(got, host))


# ---- end to end
E2E_OBJECT = T.obj(0x520, 400, 78, b"fec-0xD301.png", 200)
E2E_SLOT = 17                                                         # the slot of every FEC frame that is overwritten
E2E_FRAMES = 10                                                       # transmission frames of the cycle: 40 logical frames, 160 slots


def e2e_fec_ensemble():
    """one ensemble: a DAB+ service of 64 kbit/s, and a packet-mode sub-channel of 32 kbit/s with FEC scheme 1 that carries the
    slide ONCE in its cycle of 40 logical frames: one FEC frame and 57 slots of padding"""
    pk = synth.packetise(E2E_OBJECT[2], ADDR, sizes=(1,))
    assert E2E_SLOT < len(pk) < 80
    frames = synth.packet_fec_frames(32, [pk], n_frames=4 * E2E_FRAMES)[:4 * E2E_FRAMES]
    assert frames.shape == (4 * E2E_FRAMES, 96) and F.mark(frames.reshape(-1, 24)[102]) == 8
    service = ("Slides", 0xD301, T.E2E_SUBCH, 0, 3, 32, T.E2E_START, [(T.E2E_SCID, ADDR, synth.DSCTY_MOT, 0)], frames, 1)
    return synth.ServiceEnsemble(T.E2E_SEED, T.E2E_DABPLUS, n_frames=E2E_FRAMES, extras=False, packet_services=[service]), frames


@pytest.mark.gpu
def test_gpu_end_to_end_iq_to_fec_to_slides(pctx):
    """IQ of 16 transmission frames -> front end -> FIC pass -> fig_subchannels and fig_packet_components (fec_scheme 1) ->
    decode_ensembles_dev -> a fixed corruption of the decoded logical frames on the device (slot 17 of every FEC frame
    overwritten from a fixed seed: the Viterbi would hide channel noise at any level a short test can use) -> packet_fec_dev ->
    packet_slides_dev on the corrected frames, all on one stream, nothing waiting in between: the slide as sent.  Left out of
    the chain (d_in = the raw frames), the slide does not arrive: asserted on the reference receiver"""
    import torch
    dev = torch.device("cuda", 0)
    fps, L, FB = 16, 76 * 2552, dabgpu.NB_FRAME_BITS
    ens, frames = e2e_fec_ensemble()
    tx = ens.iq()
    c = pctx
    c.streams_reset(1)
    rx = synth.channel(tx[np.arange(fps) % E2E_FRAMES].ravel(), snr_db=20.0, rng=np.random.default_rng(12)).reshape(fps, -1)
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
    assert [sc.bitrate_kbps for sc in plan] == [64, 32] and len(comps) == 1 and comps[0].packet_address == ADDR and comps[0].fec_scheme == 1
    j = [sc.start_address for sc in plan].index(comps[0].start_address)
    br, n_cifs = plan[j].bitrate_kbps, 4 * fps
    D = dabgpu.packet_fec_delay(br)
    hist = [torch.zeros((15, sc.length * 64), dtype=torch.int8, device=dev) for sc in plan]
    outs = [torch.zeros((n_cifs, sc.bitrate_kbps * 3), dtype=torch.uint8, device=dev) for sc in plan]
    # logical frame l of the cycle is CIF 15 + l of the call (the time de-interleaver's 15); the cycle's FEC frame begins there
    noise = torch.from_numpy(np.random.default_rng(99).integers(0, 256, 24, dtype=np.uint8) | np.uint8(0x40)).to(dev)
    rows = [15 + 4 * E2E_FRAMES * k + E2E_SLOT // 4 for k in range(2) if 15 + 4 * E2E_FRAMES * k + E2E_SLOT // 4 < n_cifs]
    fixed = torch.full((n_cifs, 3 * br), FILL, dtype=torch.uint8, device=dev)
    fec_state = torch.zeros(dabgpu.packet_fec_state_bytes(br), dtype=torch.uint8, device=dev)
    fec_result = torch.zeros(48, dtype=torch.uint8, device=dev)
    state = torch.zeros(dabgpu.packet_state_bytes(), dtype=torch.uint8, device=dev)
    arena = torch.zeros(dabgpu.mot_arena_bytes(1024), dtype=torch.uint8, device=dev)
    slots = torch.full((2, 1024), FILL, dtype=torch.uint8, device=dev)
    result = torch.zeros(192, dtype=torch.uint8, device=dev)
    c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), [plan], None, [[h.data_ptr() for h in hist]],
                           [[o.data_ptr() for o in outs]], None)
    with torch.cuda.stream(torch.cuda.ExternalStream(c.stream)):      # (behind the decode call, in front of the FEC call)
        for r in rows:
            outs[j][r, 24 * (E2E_SLOT % 4):24 * (E2E_SLOT % 4) + 24] = noise
    c.packet_fec_dev([dabgpu.PacketFecEntry(outs[j].data_ptr(), 3 * br, br, 0, fixed.data_ptr(), 3 * br, None, fec_state.data_ptr(), fec_result.data_ptr())], n_cifs)
    c.packet_slides_dev([dabgpu.PacketEntry(fixed.data_ptr(), 3 * br, br, comps[0].packet_address, comps[0].fec_scheme, 0, None, state.data_ptr(),
                                            arena.data_ptr(), arena.numel(), slots.data_ptr(), 1024, 2, 0, result.data_ptr())], n_cifs)
    c.sync()                                                          # (the only wait behind the decode call)
    raw = outs[j].cpu().numpy()
    assert len(rows) == 2 and (raw[15:15 + 40].reshape(-1, 24)[np.arange(160) != E2E_SLOT] == frames.reshape(-1, 24)[np.arange(160) != E2E_SLOT]).all()
    assert (raw[15 + E2E_SLOT // 4] != frames[E2E_SLOT // 4]).any()
    fres = fec_result.cpu().numpy().view(dabgpu.PACKET_FEC_RESULT_DTYPE)
    assert int(fres["frames"][0]) == 1 and int(fres["rows_corrected"][0]) == 12 and int(fres["rows_uncorrectable"][0]) == 0, fres
    assert (fixed.cpu().numpy()[D + 15:D + 15 + 23] == frames[:23]).all()
    res = result.cpu().numpy().view(dabgpu.PACKET_RESULT_DTYPE)
    got = slots.cpu().numpy()
    header, body = E2E_OBJECT[0], E2E_OBJECT[1]
    assert int(res["mot"]["slides_written"][0]) == 1 and int(res["mot"]["groups_crc_failed"][0]) == 0 and int(res["cifs"][0]) == n_cifs, res
    rec = got[0, :32].copy().view(dabgpu.MOT_SLIDE_DTYPE)
    assert (int(rec["transport_id"][0]), int(rec["content_type"][0]), int(rec["header_bytes"][0]), int(rec["body_bytes"][0])) == (0x520, 2, len(header), len(body))
    assert got[0, 32:32 + len(header)].tobytes() == header and got[0, 32 + len(header):32 + len(header) + len(body)].tobytes() == body
    assert (got[0, 32 + len(header) + len(body):] == FILL).all() and (got[1] == FILL).all()
    # with the FEC call left out -- d_in = the raw frames, both copies of the slide in them -- it does not arrive: the reference
    lost, lc = R.Receiver(1024, ADDR, 1).call(raw, br, 2, 1024)
    assert lost == [] and int(lc["continuity_breaks"][0]) >= 2 and int(lc["packets_fec"][0]) >= 9
