"""dabgpu_mp2_follow_dev / dabgpu_mp2_follow_host (every DAB -- MPEG layer II -- sub-channel of a batch followed to checked
frames and PAD rows: header, ISO CRC over bit allocation and SCFSI, pairing of 24 kHz frames, the carry between calls)
against tests/mp2_reference.py, a bit-serial restatement of the contract in include/dabgpu_mp2_frame.h: rows, status
records, the follow record, the result record and the carry record byte for byte, every output between sentinel bytes.

CPU: the host twin on every case, the refusals, the fuzz program under the host sanitizers, the compiler's metadata of the
new kernels, and that the PAD and slideshow walks take the rows as they are.  GPU: the same cases on the device, the seams
of the lane-per-frame layout, 40 entries of mixed rates in one call, refusals with a live context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import mp2_reference as M
from conftest import ROOT
from test_device_asm import CSRC, kernel_metadata

ARG = -1
SENTINEL = 0xEE
STEREO, JOINT, DUAL, MONO = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------------------ streams
def audio(rng, B, n, mode=STEREO, mode_ext=0, lsf=False, crc=True, pads=None):
    """n audio frames as logical frames [n or 2n][3 B]"""
    frames = [synth.mp2_frame(rng, B, mode=mode, mode_ext=mode_ext, lsf=lsf, crc=crc, pad=pads[k % len(pads)] if pads else None)
              for k in range(n)]
    return np.concatenate(frames).reshape(-1, 3 * B)


def flip(frames, lf, bit):
    out = frames.copy()
    out[lf, bit >> 3] ^= 0x80 >> (bit & 7)
    return out


def alloc_bits(B, mode, lsf, mode_ext=0):
    """allocation bits of a frame (from the tables in the reference): where the SCFSI bits begin, behind bit 48"""
    channels, nbal, bound, _c = M.shape({"id": 0 if lsf else 1, "mode": mode, "mode_ext": mode_ext}, B)
    return sum(n * (2 if channels == 2 and sb < bound else 1) for sb, n in enumerate(nbal))


def build_cases():
    """name -> (B, [logical frames of call 0, of call 1, ...], expected counters of all calls summed or None)"""
    rng = np.random.default_rng(0x4D5032)
    label = synth.dls_pads(synth.dls_segments(b"layer two", toggle=1), length_index=3)
    cases = {}
    # the small table (c = 2) and the large one (c = 4), every joint-stereo bound
    for name, B, mode, ext in [("32 mono", 32, MONO, 0), ("64 stereo", 64, STEREO, 0), ("96 stereo", 96, STEREO, 0),
                               ("56 mono", 56, MONO, 0), ("128 joint bound 4", 128, JOINT, 0), ("128 joint bound 8", 128, JOINT, 1),
                               ("128 joint bound 12", 128, JOINT, 2), ("128 joint bound 16", 128, JOINT, 3),
                               ("384 stereo", 384, STEREO, 0), ("192 dual", 192, DUAL, 0), ("96 joint small table", 96, JOINT, 3)]:
        cases[name] = (B, [audio(rng, B, 5, mode, ext, pads=label)], dict(frames=5, header_errors=0, crc_failed=0, frames_no_crc=0))
    # 24 kHz: both phases, a call boundary that splits a pair
    for B in (8, 64, 160):
        mode = [STEREO, JOINT, MONO][B % 3]
        a = audio(rng, B, 6, mode, 1, lsf=True, pads=label if B > 8 else None)
        cases["24 kHz %d phase 0" % B] = (B, [a], dict(frames=6, header_errors=0, crc_failed=0, frames_no_crc=0))
        cases["24 kHz %d phase 1" % B] = (B, [a[1:]], dict(frames=5))
        cases["24 kHz %d split pair" % B] = (B, [a[:5], a[5:]], dict(frames=6, crc_failed=0, header_errors=0))
        cases["24 kHz %d phase 1 split pair" % B] = (B, [a[1:4], a[4:6], a[6:]], dict(frames=5))
    # every split of a 7-frame run into two calls
    run48, run24 = audio(rng, 64, 7, STEREO, pads=label), audio(rng, 64, 4, JOINT, 2, lsf=True, pads=label)[:7]
    for k in range(8):
        cases["48 kHz run split at %d" % k] = (64, [run48[:k], run48[k:]], dict(frames=7, crc_failed=0, header_errors=0))
        cases["24 kHz run split at %d" % k] = (64, [run24[:k], run24[k:]], dict(frames=3, crc_failed=0, header_errors=0))
        cases["24 kHz phase 1 run split at %d" % k] = (64, [run24[1:][:k], run24[1:][k:]], dict(frames=2, crc_failed=0, header_errors=0))
    # corruptions of frame 2 of five: 48 kHz joint stereo at 128, and the second frame of three at 24 kHz
    base = audio(rng, 128, 5, JOINT, 1, pads=label)
    ab = alloc_bits(128, JOINT, False, 1)
    lost = lambda **kw: dict(dict(frames=5, header_errors=0, crc_failed=0, frames_no_crc=0), **kw)
    cases["flip sync"] = (128, [flip(base, 2, 5)], lost(header_errors=1))
    cases["flip layer"] = (128, [flip(base, 2, 13)], lost(header_errors=1))
    cases["flip mode (covered by the CRC)"] = (128, [flip(base, 2, 24)], lost(crc_failed=1))
    cases["flip allocation"] = (128, [flip(base, 2, 48 + 2)], lost(crc_failed=1))
    cases["flip last allocation bit"] = (128, [flip(base, 2, 48 + ab - 1)], lost(crc_failed=1))
    cases["flip first scfsi bit"] = (128, [flip(base, 2, 48 + ab)], lost(crc_failed=1))
    cases["flip crc"] = (128, [flip(base, 2, 32 + 7)], lost(crc_failed=1))
    cases["flip protection bit"] = (128, [flip(base, 2, 15)], lost(frames_no_crc=1))
    cases["unharmed"] = (128, [base], lost())
    cases["flip body"] = (128, [flip(base, 2, 8 * 90 + 3)], lost())        # (behind the protected bits, in front of the lifted tail)
    cases["flip copyright (the header check does not look at it, the CRC covers it)"] = (128, [flip(base, 2, 28)], lost(crc_failed=1))
    low = audio(rng, 64, 3, STEREO, lsf=True, pads=label)
    cases["24 kHz flip allocation"] = (64, [flip(low, 2, 48 + 9)], dict(frames=3, crc_failed=1, header_errors=0))
    cases["24 kHz flip second half header-like bytes"] = (64, [flip(low, 3, 3)], dict(frames=3, crc_failed=0, header_errors=0))
    cases["24 kHz flip sync"] = (64, [flip(low, 2, 0)], dict(frames=3, crc_failed=0, header_errors=1))
    # a bit-rate index that names another rate: every header fails, no rate, no rows
    wrong = audio(rng, 160, 4, STEREO)
    wrong[:, 2] = (wrong[:, 2] & 0x0F) | (8 << 4)
    cases["wrong bit-rate index"] = (160, [wrong], dict(frames=0))
    one_wrong = audio(rng, 160, 4, STEREO)
    one_wrong[1, 2] = (one_wrong[1, 2] & 0x0F) | (8 << 4)
    cases["one wrong bit-rate index"] = (160, [one_wrong], dict(frames=4, header_errors=1, crc_failed=0))
    cases["all 0xFF"] = (64, [np.full((4, 192), 0xFF, np.uint8)], dict(frames=0))
    cases["all zero"] = (64, [np.zeros((4, 192), np.uint8)], dict(frames=0))
    cases["all zero behind a synced call"] = (64, [run48[:3], np.zeros((2, 192), np.uint8), np.zeros((2, 192), np.uint8), run48[3:5]],
                                              dict(frames=3 + 2 + 0 + 3, header_errors=2 + 1, dropped=1))   # (the held zero frame: a row)
    # a frame of the other ID in mid-stream
    other = run48[:5].copy()
    other[2] = audio(rng, 64, 1, STEREO, lsf=True)[0]
    cases["24 kHz header inside 48 kHz"] = (64, [other], dict(frames=5, header_errors=1, crc_failed=0))
    other = run24[:6].copy()
    other[2] = run48[0]
    cases["48 kHz header inside 24 kHz"] = (64, [other], dict(frames=3, header_errors=1, crc_failed=0))
    cases["as many 48 kHz hits as 24 kHz: 48 kHz"] = (64, [np.concatenate([run48[:1], run24[:2]])], dict(frames=3, header_errors=2))
    # no CRC (what the synthetic multiplex has sent so far): counted, no PAD
    cases["protection bit 1"] = (192, [audio(rng, 192, 4, STEREO, crc=False)], dict(frames=4, frames_no_crc=4, crc_failed=0))
    cases["nothing"] = (64, [run48[:0]], dict(frames=0))
    return cases


CASES = build_cases()


# ------------------------------------------------------------------------------------------------------------ memory
class HostMemory:
    def __init__(self):
        self.keep = []

    def put(self, a, align=16):
        raw = np.zeros(a.nbytes + align, np.uint8)
        off = (-raw.ctypes.data) % align
        buf = raw[off:off + a.nbytes]
        buf[:] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.keep.append(raw)
        return buf, buf.ctypes.data

    def get(self, buf):
        return np.array(buf)

    def follow(self, entries, n_cifs):
        return dabgpu.lib().dabgpu_mp2_follow_host((dabgpu.Mp2Entry * max(len(entries), 1))(*entries), len(entries), n_cifs)


class DeviceMemory:
    def __init__(self, ctx):
        self.ctx = ctx

    def put(self, a, align=16):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        return t, t.data_ptr()

    def get(self, buf):
        return buf.cpu().numpy()

    def follow(self, entries, n_cifs):
        try:
            self.ctx.mp2_follow_dev(entries, n_cifs)
        except dabgpu.DabGpuError as e:
            return e.status
        self.ctx.sync()
        return 0


def call(mem, specs, n_cifs, mutate=None):
    """specs: dicts {B, frames [n_cifs][3 B], carry (bytes or None), pad (extra in_stride)} -> (rc, [outputs per entry]):
    every output lies in sentinel bytes; outputs as numpy"""
    entries, bufs = [], []
    for sp in specs:
        B, stride = sp["B"], 3 * sp["B"] + sp.get("pad", 0)
        src = np.full((max(n_cifs, 1), stride), 0x55, np.uint8)
        src[:n_cifs, :3 * B] = sp["frames"]
        cb = M.carry_bytes(B)
        b_in, p_in = mem.put(src)
        b_ci, p_ci = mem.put(np.frombuffer(sp["carry"], np.uint8)) if sp.get("carry") is not None else (None, None)
        b_co, p_co = mem.put(np.full(cb + 16, SENTINEL, np.uint8))
        off = sp.get("rows_off", 0)                                    # d_rows has no alignment to keep
        b_rows, p_rows = mem.put(np.full(4 + (n_cifs + 2) * 220, SENTINEL, np.uint8))
        p_rows += off
        b_st, p_st = mem.put(np.full((n_cifs + 2) * 64, SENTINEL, np.uint8))
        b_fo, p_fo = mem.put(np.full(32 + 16, SENTINEL, np.uint8))
        b_re, p_re = mem.put(np.full(64 + 16, SENTINEL, np.uint8))
        entries.append(dabgpu.Mp2Entry(p_in, stride, B, p_ci, p_co, p_rows, p_st, p_fo, p_re))
        bufs.append((b_co, b_rows, b_st, b_fo, b_re, b_in, b_ci))
    if mutate:
        mutate(entries)
    rc = mem.follow(entries, n_cifs)
    outs = []
    for (b_co, b_rows, b_st, b_fo, b_re, _i, _c), sp in zip(bufs, specs):
        off, raw = sp.get("rows_off", 0), mem.get(b_rows)
        assert (raw[:off] == SENTINEL).all() and (raw[off + (len(raw) - 4):] == SENTINEL).all()
        outs.append(dict(carry=mem.get(b_co), rows=raw[off:off + len(raw) - 4].reshape(-1, 220), status=mem.get(b_st).reshape(-1, 64),
                         follow=mem.get(b_fo), result=mem.get(b_re), cb=M.carry_bytes(sp["B"])))
    return rc, outs


def untouched(out):
    return all((out[k] == SENTINEL).all() for k in ("carry", "rows", "status", "follow", "result"))


def compare(out, want, what):
    """one entry's outputs against the reference's, and the sentinel bytes around them"""
    n = len(want["rows"])
    assert out["follow"][:32].view(np.int32).tolist() == want["follow"].tolist(), what
    assert out["result"][:64].view(np.int32).tolist() == want["result"].tolist(), what
    assert out["carry"][:out["cb"]].tobytes() == want["carry"], what
    assert (out["rows"][:n] == want["rows"]).all(), what
    assert (out["status"][:n].reshape(-1).view(np.int32).reshape(n, 16) == want["status"]).all(), what
    # rows beyond the count are not written; nothing is written behind any record
    assert (out["rows"][n:] == SENTINEL).all() and (out["status"][n:] == SENTINEL).all(), what
    assert (out["follow"][32:] == SENTINEL).all() and (out["result"][64:] == SENTINEL).all() and (out["carry"][out["cb"]:] == SENTINEL).all(), what


RESULT_FIELDS = dabgpu.MP2_RESULT_DTYPE.names


def run_case(mem, name):
    B, calls, expect = CASES[name]
    carry, total, good_rows = None, dict.fromkeys(RESULT_FIELDS, 0), 0
    for k, frames in enumerate(calls):
        rc, (out,) = call(mem, [dict(B=B, frames=frames, carry=carry, pad=[0, 8, 3][k % 3], rows_off=(k + 1) % 4)], len(frames))
        assert rc == 0, name
        want = M.follow(list(frames), B, carry)
        compare(out, want, (name, k))
        carry = want["carry"]
        rec = out["result"][:64].view(dabgpu.MP2_RESULT_DTYPE)[0]
        for f in ("frames", "header_errors", "crc_failed", "frames_no_crc", "dropped"):
            total[f] += int(rec[f])
        good_rows += int((want["status"][:, 4] == 1).sum()) if len(want["status"]) else 0
    for f, v in (expect or {}).items():
        assert total[f] == v, (name, f, total)
    assert good_rows == total["frames"] - total["header_errors"] - total["crc_failed"] - total["frames_no_crc"], name
    return total


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_are_exported_and_typed(built):
    L = dabgpu.lib()
    for name in ("dabgpu_mp2_follow_dev", "dabgpu_mp2_follow_host", "dabgpu_mp2_carry_bytes"):
        assert name in dabgpu.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.dabgpu_abi_version() == 6 == dabgpu.ABI_VERSION           # (pinned by tests/test_abi_cpu.py: not bumped)
    assert C.sizeof(dabgpu.Mp2Entry) == 72 and dabgpu.MP2_RESULT_DTYPE.itemsize == 64
    assert (dabgpu.MP2_ROW_BYTES, dabgpu.MP2_PAD_KBPS) == (220, 16) == (M.ROW_BYTES, 220 * 8 // 110)
    hdr = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    assert "#define DABGPU_MP2_ROW_BYTES 220" in hdr and "#define DABGPU_MP2_PAD_KBPS 16" in hdr
    assert hasattr(dabgpu.Context, "mp2_follow_dev")


def test_binding_matches_the_header(tmp_path):
    fields = [f for f, _ in dabgpu.Mp2Entry._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dabgpu.h"', 'int main(void) {',
             '  printf("%zu", sizeof(dabgpu_mp2_entry));']
    lines += ['  printf(" %%zu", offsetof(dabgpu_mp2_entry, %s));' % f for f in fields]
    lines += ['  printf("\\n%zu", sizeof(dabgpu_mp2_result));']
    lines += ['  printf(" %%zu", offsetof(dabgpu_mp2_result, %s));' % f for f in RESULT_FIELDS]
    lines += ['  return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(tmp_path / "layout")])
    entry, result = [[int(v) for v in line.split()] for line in subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")]
    assert entry == [C.sizeof(dabgpu.Mp2Entry)] + [getattr(dabgpu.Mp2Entry, f).offset for f in fields]
    assert result == [64] + [dabgpu.MP2_RESULT_DTYPE.fields[f][1] for f in RESULT_FIELDS]


def test_carry_bytes(built):
    for br in range(8, 385, 8):
        assert dabgpu.mp2_carry_bytes(br) == M.carry_bytes(br) >= 16 + 3 * br and dabgpu.mp2_carry_bytes(br) % 16 == 0
    for br in (0, -8, 4, 12, 385, 392, 512):
        assert dabgpu.mp2_carry_bytes(br) == 0


def test_the_two_crc_implementations_of_the_test_side_agree():
    """synth.mp2_frame (a byte table) and the reference (a shift register) share no code: every frame the one builds the
    other finds good, for every legal (rate, mode, ID)"""
    rng = np.random.default_rng(5)
    n = 0
    for lsf, rates in ((False, synth.MP2_RATES_48K[1:]), (True, synth.MP2_RATES_24K[1:])):
        for B in rates:
            for mode in range(4):
                if not lsf and ((B in M.MONO_ONLY and mode != MONO) or (B in M.TWO_CHANNEL_ONLY and mode == MONO)):
                    continue
                f = synth.mp2_frame(rng, B, mode=mode, mode_ext=int(rng.integers(4)), lsf=lsf)
                kind, c = M.check_frame(bytes(f), B, 0 if lsf else 1)
                assert kind == M.GOOD and c == synth.mp2_scf_crc_bytes(B, mode, lsf), (B, mode, lsf)
                n += 1
    assert n == (4 * 1 + 6 * 4 + 4 * 3) + 14 * 4
    assert M.crc_bit_serial(M.bits_of(b"123456789")) == 0xAEE7          # CRC-16/CMS: 0x8005, start 0xFFFF, no reflection


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_reference(built, name):
    run_case(HostMemory(), name)


def test_a_flipped_body_bit_changes_nothing(built):
    """a bit between the protected front and the lifted tail: every output is byte for byte that of the unharmed stream"""
    (B, (clean,), _e), (_B, (harmed,), _e2) = CASES["unharmed"], CASES["flip body"]
    assert (clean != harmed).sum() == 1
    a, b = (call(HostMemory(), [dict(B=B, frames=f)], len(f))[1][0] for f in (clean, harmed))
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("carry", "rows", "status", "follow", "result"))
    assert 8 * 6 + alloc_bits(128, JOINT, False, 1) + 2 * 2 * 27 < 8 * 90 < 8 * (384 - 2 - 4 - 196)


def test_every_legal_rate_mode_and_id_on_the_host(built):
    rng = np.random.default_rng(6)
    for lsf, rates in ((False, synth.MP2_RATES_48K[1:]), (True, synth.MP2_RATES_24K[1:])):
        for B in rates:
            for mode in range(4):
                if not lsf and ((B in M.MONO_ONLY and mode != MONO) or (B in M.TWO_CHANNEL_ONLY and mode == MONO)):
                    continue
                frames = audio(rng, B, 2, mode, int(rng.integers(4)), lsf=lsf)
                rc, (out,) = call(HostMemory(), [dict(B=B, frames=frames)], len(frames))
                want = M.follow(list(frames), B)
                compare(out, want, (B, mode, lsf))
                assert rc == 0 and want["result"][8:13].tolist() == [2, 0, 0, 0, 0] and want["result"][3] == mode


def test_a_foreign_carry_record_is_a_fresh_start(built):
    B, frames = 64, CASES["48 kHz run split at 0"][1][1][:3]
    good = M.follow(list(CASES["24 kHz 64 split pair"][1][0]), B)["carry"]
    assert good[:16] == np.array([1, 1, 2, M.MAGIC], np.int32).tobytes()
    rng = np.random.default_rng(8)
    records = [bytes(M.carry_bytes(B)), bytes(rng.integers(0, 256, M.carry_bytes(B), dtype=np.uint8))]
    for words in ([1, 1, 2, 0], [2, 0, 1, M.MAGIC], [1, 2, 2, M.MAGIC], [1, 0, 3, M.MAGIC], [1, 0, 0, M.MAGIC], [0, 1, 2, M.MAGIC],
                  [1, 1, 1, M.MAGIC], [-1, 0, 0, M.MAGIC]):
        records.append(np.array(words, np.int32).tobytes() + good[16:])
    fresh = M.follow(list(frames), B)
    for rec in records:
        rc, (out,) = call(HostMemory(), [dict(B=B, frames=frames, carry=rec)], 3)
        assert rc == 0
        compare(out, M.follow(list(frames), B, rec), rec[:16])
        compare(out, fresh, rec[:16])
    # the record this library wrote is not: its held half comes first
    rc, (out,) = call(HostMemory(), [dict(B=B, frames=frames, carry=good)], 3)
    compare(out, M.follow(list(frames), B, good), "good")
    assert out["result"][:64].view(dabgpu.MP2_RESULT_DTYPE)["frames"][0] == 4


def _entry(bitrate=64, d_in=0x10000, stride=None, cin=0x20000, cout=0x30000, rows=0x40000, status=0x50000, follow=0x60000, result=0x70000):
    return dabgpu.Mp2Entry(d_in, 3 * bitrate if stride is None else stride, bitrate, cin, cout, rows, status, follow, result)


#: (what is wrong, how a good table is changed) -- each refused with DABGPU_ERR_ARG before anything is done
def _set(i, **kw):
    def m(entries):
        for k, v in kw.items():
            setattr(entries[i], k, v(getattr(entries[i], k)) if callable(v) else v)
    return m


BAD_ENTRIES = [
    ("bit rate no multiple of 8", _set(1, bitrate_kbps=68)),
    ("bit rate 0", _set(0, bitrate_kbps=0)),
    ("bit rate negative", _set(0, bitrate_kbps=-64)),
    ("bit rate above 384", _set(1, bitrate_kbps=392, in_stride=4096)),
    ("in_stride below bitrate * 3", _set(1, in_stride=lambda v: 191)),
    ("carry in == out", lambda e: setattr(e[1], "d_carry_in", e[1].d_carry_out)),
    ("carry in overlaps out", lambda e: setattr(e[0], "d_carry_in", e[0].d_carry_out + 16)),
    ("carry out off its boundary", _set(1, d_carry_out=lambda v: v + 8)),
    ("carry in off its boundary", lambda e: setattr(e[0], "d_carry_in", e[1].d_carry_out + 4)),
    ("null carry out", _set(0, d_carry_out=None)),
    ("null input", _set(1, d_in=None)),
    ("null rows", _set(0, d_rows=None)),
    ("null status", _set(1, d_status=None)),
    ("null follow", _set(0, d_follow=None)),
    ("null result", _set(1, d_result=None)),
    ("status off its boundary", _set(1, d_status=lambda v: v + 2)),
    ("follow off its boundary", _set(0, d_follow=lambda v: v + 1)),
    ("result off its boundary", _set(1, d_result=lambda v: v + 2)),
]


def refusal_specs():
    return [dict(B=64, frames=CASES["64 stereo"][1][0][:4]), dict(B=64, frames=CASES["48 kHz run split at 0"][1][1][:4])]


def check_refusals(mem):
    for what, m in BAD_ENTRIES:
        rc, outs = call(mem, refusal_specs(), 4, mutate=m)
        assert rc == ARG, what
        assert all(untouched(o) for o in outs), what                 # the good entry in front of the bad one too
    rc, outs = call(mem, refusal_specs(), 4)
    assert rc == 0 and not any(untouched(o) for o in outs)


def test_refusals_of_the_host_twin(built):
    check_refusals(HostMemory())
    L = dabgpu.lib()
    good = (dabgpu.Mp2Entry * 1)(_entry())
    assert L.dabgpu_mp2_follow_host(None, 1, 4) == ARG                   # null table
    assert L.dabgpu_mp2_follow_host(good, -1, 4) == ARG                  # negative counts
    assert L.dabgpu_mp2_follow_host(good, 1, -1) == ARG
    assert L.dabgpu_mp2_follow_host(good, 1, (1 << 28) + 1) == ARG           # n_cifs above 2^28 (before any pointer is looked at)
    assert L.dabgpu_mp2_follow_dev(None, good, 1, (1 << 28) + 1, None) == ARG
    assert L.dabgpu_mp2_follow_host(None, 0, 4) == 0                     # nothing to do is not an error
    assert L.dabgpu_mp2_follow_dev(None, good, 1, 4, None) == ARG        # no context
    rc, (out,) = call(HostMemory(), [dict(B=64, frames=np.zeros((0, 192), np.uint8))], 0, mutate=_set(0, d_in=None))
    assert rc == 0 and out["follow"][:4].view(np.int32)[0] == 0          # d_in may be NULL with n_cifs = 0


# ---- the rows under the two walks
SLIDE = bytes(np.random.default_rng(77).integers(0, 256, 700, dtype=np.uint8))
LABEL = "Jetzt: Sinfonie Nr. 5 – Allegro".encode("utf-8")


NO_XPAD = synth.pad_field(b"", 0, 0)                                 # F-PAD alone, saying so


def label_and_slide_pads(n, sizes=(58,)):
    """n PADs carrying LABEL (over and over) and SLIDE (once) as synth.pack_pads lays them out"""
    header = synth.slide_header(len(SLIDE), b"two.jpg")
    mot = synth.mot_object_groups(0x1234, header, SLIDE, 120)
    dls = synth.dls_segments(LABEL, toggle=1)
    fields = synth.merge_fields(synth.mot_fields(mot, 7), synth.dls_fields(dls * 4, 3))
    pads = synth.fields_pads(fields)
    assert len(pads) <= n, len(pads)
    return [p if p is not None else NO_XPAD for p in pads] + [NO_XPAD] * (n - len(pads)), header


def walk_rows(rows, status, follow, n_rows):
    """pad_labels_host and mot_slides_host over rows of the layer-II follow call -> (label text, counters, slides, counters)"""
    hm = HostMemory()
    _r, p_rows = hm.put(rows)
    _s, p_st = hm.put(status)
    _f, p_fo = hm.put(follow)
    b_so, p_so = hm.put(np.zeros(dabgpu.pad_state_bytes(), np.uint8))
    b_lab, p_lab = hm.put(np.zeros(144, np.uint8))
    b_res, p_res = hm.put(np.zeros(64, np.uint8))
    dabgpu.pad_labels_host([dabgpu.PadEntry(p_rows, 220, p_st, p_fo, dabgpu.MP2_PAD_KBPS, n_rows, None, p_so, p_lab, p_res)])
    arena = dabgpu.mot_arena_bytes(4096)
    b_ms, p_ms = hm.put(np.zeros(dabgpu.mot_state_bytes(), np.uint8))
    b_ar, p_ar = hm.put(np.zeros(arena, np.uint8))
    b_sl, p_sl = hm.put(np.zeros(2 * 4096, np.uint8))
    b_mr, p_mr = hm.put(np.zeros(128, np.uint8))
    dabgpu.mot_slides_host([dabgpu.MotEntry(p_rows, 220, p_st, p_fo, dabgpu.MP2_PAD_KBPS, n_rows, None, p_ms, p_ar, arena, p_sl, 4096, 2, 0, p_mr)])
    return (b_lab.view(dabgpu.PAD_LABEL_DTYPE)[0], b_res.view(dabgpu.PAD_RESULT_DTYPE)[0], np.array(b_sl).reshape(2, 4096),
            b_mr.view(dabgpu.MOT_RESULT_DTYPE)[0])


def slide_of(slot):
    rec = slot[:32].view(dabgpu.MOT_SLIDE_DTYPE)[0]
    h, b = int(rec["header_bytes"]), int(rec["body_bytes"])
    return bytes(slot[32:32 + h]), bytes(slot[32 + h:32 + h + b])


@pytest.mark.parametrize("B,mode,lsf", [(128, JOINT, False), (64, STEREO, False), (64, STEREO, True), (32, MONO, False)])
def test_the_walks_take_the_rows_and_the_generous_x_costs_nothing(built, B, mode, lsf):
    """a label and a slide in the PAD of layer-II frames whose bodies are random: the rows hold x = min(196, L - 8 - c) bytes
    of which the PAD is a part, the rest audio; both walks read only what the content indicators announce -- nothing is
    malformed, label and slide come out as sent"""
    rng = np.random.default_rng(B + 2 * lsf)
    pads, header = label_and_slide_pads(40)
    frames = audio(rng, B, 40, mode, 2, lsf=lsf, pads=pads)
    rc, (out,) = call(HostMemory(), [dict(B=B, frames=frames)], len(frames))
    want = M.follow(list(frames), B)
    compare(out, want, B)
    x = min(196, len(frames[0]) * (2 if lsf else 1) - 8 - synth.mp2_scf_crc_bytes(B, mode, lsf))
    assert (want["status"][:, 6] == x + 6).all() and x > max(len(p) for p in pads if p) - 2
    lab, res, slides, mres = walk_rows(out["rows"], out["status"], out["follow"][:32], len(frames) + 1)
    assert dabgpu.pad_label_utf8(lab) == LABEL.decode("utf-8")
    assert int(res["aus"]) == 40 and int(res["aus_lost"]) == 0 and int(res["pad_malformed"]) == 0 and int(res["groups_crc_failed"]) == 0
    assert int(mres["objects_completed"]) == 1 and int(mres["slides_written"]) == 1 and int(mres["pad_malformed"]) == 0
    assert slide_of(slides[0]) == (header, SLIDE)
    # a frame that fails its CRC is one lost access unit for both walks
    rc, (out,) = call(HostMemory(), [dict(B=B, frames=flip(frames, 0, 48 + 1))], len(frames))
    lab, res, _sl, mres = walk_rows(out["rows"], out["status"], out["follow"][:32], len(frames) + 1)
    assert int(res["aus_lost"]) == 1 == int(mres["aus_lost"])


def test_frame_fuzz_under_sanitizers(tmp_path):
    """tests/mp2_frame_fuzz.cpp: 200 000 random, valid and mutated frames of every legal length, every logical frame in an
    exactly sized heap block, built with the host compiler under AddressSanitizer and UBSan and run as a child process"""
    exe = str(tmp_path / "mp2_frame_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mp2_frame_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "200000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "frames=200000" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
    assert got["outside"] == 0 and min(got["good"], got["header"], got["no_crc"], got["crc_failed"]) > 1000 and got["rows"] == got["good"], r.stdout


def test_kernels_use_no_scratch_and_spill_nothing(built, tmp_path):
    """the metadata of mp2_kernels.o, the object the library is linked from: two kernels, no scratch, no spills (the
    allocation-width lookups are comparisons, the bit reader indexes LDS)"""
    obj = os.path.join(CSRC, "mp2_kernels.o")
    llvm = "/opt/rocm/lib/llvm/bin/"
    if not (os.path.exists(obj) and os.path.exists(llvm + "llvm-readelf")):
        pytest.fail("toolchain or mp2_kernels.o missing")
    fat, co = str(tmp_path / "mp2.fat"), str(tmp_path / "mp2.co")
    subprocess.check_call([llvm + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([llvm + "clang-offload-bundler", "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    md = kernel_metadata(subprocess.check_output([llvm + "llvm-readelf", "--notes", co], text=True))
    assert len(md) == 2 and any("mp2_rate_kernel" in k for k in md) and any("mp2_frame_kernel" in k for k in md), list(md)
    for k, v in md.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_count"] <= 128 and v.get("agpr_count", 0) == 0, (k, v)


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def mctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.gpu
def test_gpu_every_case_equals_the_reference(mctx):
    mem = DeviceMemory(mctx)
    for name in CASES:
        run_case(mem, name)


@pytest.fixture(scope="module")
def long_runs():
    """196 logical frames at 48 kHz and 132 at 24 kHz with their PAD, some frames damaged: shared by the seam tests"""
    rng = np.random.default_rng(0x5EA)
    pads, _h = label_and_slide_pads(131)
    r48 = audio(rng, 96, 196, STEREO, pads=pads)
    r24 = audio(rng, 48, 66, JOINT, 0, lsf=True, pads=pads)
    for lf, bit in ((0, 50), (62, 3), (63, 33), (64, 15), (65, 49), (127, 60), (128, 1), (129, 52), (130, 40)):
        r48, r24 = flip(r48, lf, bit), flip(r24, lf, bit)
    return r48, r24


@pytest.mark.gpu
@pytest.mark.parametrize("n_cifs", [1, 2, 63, 64, 65, 130])
def test_gpu_seams_of_the_lane_per_frame_layout(mctx, long_runs, n_cifs):
    """n_cifs around one and two chunks of 64 frames, at 48 kHz and at 24 kHz in both phases, fresh and behind a carry that
    holds a frame (so the rows number n_cifs + 1 at 48 kHz): one call of nine entries, each against the reference"""
    r48, r24 = long_runs
    held48 = struct_carry(0, 1, 0, r48[0])                               # a held frame that is not synced: a row of its own
    held24 = M.follow([r24[0]], 48)["carry"]
    assert held24[:8] == np.array([1, 1], np.int32).tobytes()
    specs = [dict(B=96, frames=r48[:n_cifs]), dict(B=96, frames=r48[1:1 + n_cifs], carry=held48, pad=8),
             dict(B=48, frames=r24[:n_cifs], pad=5), dict(B=48, frames=r24[1:1 + n_cifs], pad=16),
             dict(B=48, frames=r24[1:1 + n_cifs], carry=held24), dict(B=48, frames=r24[2:2 + n_cifs], carry=held24),
             dict(B=96, frames=r48[n_cifs // 2:][:n_cifs], pad=1), dict(B=48, frames=np.zeros((n_cifs, 144), np.uint8)),
             dict(B=96, frames=np.zeros((n_cifs, 288), np.uint8), carry=M.follow(list(r48[:2]), 96)["carry"])]
    rc, outs = call(DeviceMemory(mctx), specs, n_cifs)
    assert rc == 0
    rows = []
    for k, (sp, out) in enumerate(zip(specs, outs)):
        want = M.follow(list(sp["frames"]), sp["B"], sp.get("carry"))
        compare(out, want, (n_cifs, k))
        rows.append(len(want["rows"]))
    assert rows[0] == n_cifs and rows[1] == n_cifs + 1 and rows[2] == n_cifs // 2 and rows[4] == (n_cifs + 1) // 2 and rows[7] == 0
    assert rows[8] == n_cifs                                             # (a synced carry keeps its rate through a call without a hit)
    host = call(HostMemory(), specs, n_cifs)[1]
    for g, h in zip(outs, host):
        assert all(g[k].tobytes() == h[k].tobytes() for k in ("carry", "rows", "status", "follow", "result"))


def struct_carry(synced, held, rate, frame):
    rec = np.array([synced, held, rate, M.MAGIC], np.int32).tobytes() + bytes(frame)
    return rec + bytes(M.carry_bytes(len(frame) // 3) - len(rec))


@pytest.mark.gpu
def test_gpu_forty_entries_of_mixed_rates_in_one_call(mctx):
    """40 entries in ONE call -- every 48 kHz rate, every 24 kHz rate, modes in rotation, odd strides, some with a held
    half, some damaged, some silent, the rows of three in four off their 4-byte boundary by 1, 2 or 3 bytes -- each against the
    reference"""
    rng = np.random.default_rng(40)
    n_cifs, specs = 10, []
    for k in range(40):
        lsf = k % 3 == 1
        rates = synth.MP2_RATES_24K[1:] if lsf else synth.MP2_RATES_48K[1:]
        B = rates[(k * 5) % 14]
        mode = k % 4
        if not lsf and B in M.MONO_ONLY:
            mode = MONO
        if not lsf and B in M.TWO_CHANNEL_ONLY and mode == MONO:
            mode = JOINT
        frames = audio(rng, B, 12, mode, k % 4, lsf=lsf, crc=k % 11 != 10)
        sp = dict(B=B, pad=[0, 8, 3, 16][k % 4], rows_off=(k // 2) % 4)  # (rows on and off a 4-byte boundary: word and byte stores)
        if lsf and k % 2:
            sp["carry"], frames = M.follow([frames[0]], B)["carry"], frames[1:]
        if k % 7 == 3:
            frames = flip(frames, 4, 48 + k)
        if k == 20:
            frames = np.zeros_like(frames)
        sp["frames"] = frames[:n_cifs]
        specs.append(sp)
    rc, outs = call(DeviceMemory(mctx), specs, n_cifs)
    assert rc == 0
    seen = set()
    for k, (sp, out) in enumerate(zip(specs, outs)):
        want = M.follow(list(sp["frames"]), sp["B"], sp.get("carry"))
        compare(out, want, k)
        seen.add((int(want["result"][0]), int(want["result"][5])))
    assert seen >= {(1, 0), (0, 0), (0, 1), (-1, 1)}


@pytest.mark.gpu
def test_gpu_refused_calls_leave_every_output_alone(mctx):
    check_refusals(DeviceMemory(mctx))
    with pytest.raises(dabgpu.DabGpuError):
        mctx.mp2_follow_dev([dabgpu.Mp2Entry()], 4)
    mctx.mp2_follow_dev([], 4)                                           # nothing to do is not an error
