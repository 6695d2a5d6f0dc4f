"""dabgpu_mp2_subbands_dev / dabgpu_mp2_subbands_host (every checked frame of every followed layer-II sub-channel taken on to
sub-band samples and an audio level record: bit allocation, SCFSI, scale factors, the grouped code words, requantisation
and scaling -- the whole layer-II decoder but its synthesis filter) against tests/mp2_audio_reference.py, a bit-serial
restatement of the contract in include/dabgpu_mp2_audio.h, and against the truth synth.mp2_audio_pack returns with every
frame.  Sub-band values and peak are held bit for bit, power to the worst case of summing 1152 non-negative terms in any
order, records and counters exactly; every output lies between sentinel bytes.

CPU: the host twin on every case, the refusals, the fuzz program under the host sanitizers, the compiler's metadata of the
new kernels.  GPU: the same cases on the device in one call each, the seams of the wave-per-frame layout, 40 entries of mixed
rates chained behind the follow call on one stream, refusals with a live context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import mp2_audio_reference as A
import mp2_reference as M
import test_mp2_follow as T
from conftest import ROOT
from test_device_asm import CSRC, kernel_metadata

ARG = -1
SENTINEL = 0xEE
STEREO, JOINT, DUAL, MONO = 0, 1, 2, 3
U = 2.0 ** -24
#: value against truth: two rounded constants and two rounded products, (1 + u)^4 - 1 <= 5 u
VALUE_TOL = 5 * U
#: power against the float64 sum of the definition's squares: 1152 non-negative terms summed in any order, each the square
#: of a value within 5 u
POWER_TOL = 1152 * U + 2 * 5 * U
LEVEL, RESULT = dabgpu.MP2_LEVEL_DTYPE, dabgpu.MP2_AUDIO_RESULT_DTYPE
FRAME_VALUES = 2 * 36 * 32


# ------------------------------------------------------------------------------------------------------------ frames
def legal(B, mode, lsf):
    return lsf or not ((B in M.MONO_ONLY and mode != MONO) or (B in M.TWO_CHANNEL_ONLY and mode == MONO))


def logical(frames, B):
    return np.concatenate(frames).reshape(-1, 3 * B)


def chosen(B, mode, lsf, cells, mode_ext=0, rng=None, codes=None, fit=True):
    """a frame whose active cells are exactly `cells`: {(sb, ch): (a, scfsi, (index of part 0, 1, 2), samples [36])}"""
    alloc, scfsi = np.zeros((2, 32), np.int64), np.zeros((2, 32), np.int64)
    scf, samples = np.zeros((2, 32, 3), np.int64), np.zeros((2, 36, 32), np.int64)
    for (sb, ch), (a, si, idx, smp) in cells.items():
        alloc[ch][sb], scfsi[ch][sb], scf[ch][sb], samples[ch, :, sb] = a, si, idx, smp
    return synth.mp2_audio_pack(rng or np.random.default_rng(sum(B + 7 * sb + ch for sb, ch in cells)), B, mode, mode_ext, lsf,
                                alloc, scfsi, scf, samples, codes=codes, fit=fit)


def ramp(n, start=0, count=36, step=1):
    """sample codes start, start + step, ... of a class of n levels, the all-ones code n included"""
    return [(start + step * k) % (n + 1) for k in range(count)]


def build_cases():
    """name -> dict(B, frames [4][3 B] logical frames, lsf, carry, truth [rows][2][36][32] or None, kinds [rows])"""
    rng = np.random.default_rng(0x4D503241)
    cases = {}

    def add(name, B, lsf, made, carry=None, kinds=None, lf=None):
        frames = logical([f for f, _t in made], B) if lf is None else lf
        assert len(frames) == 4, name
        cases[name] = dict(B=B, lsf=lsf, frames=frames, carry=carry, truth=[t for _f, t in made] if lf is None else None, kinds=kinds)

    # ---- values: the grouped classes, every code, those at and above n^3 too.  24 kHz single channel: sub-bands 11 .. 29 hold
    # the classes 3, 5, 9 at a = 1, 2, 3; 19 cells carry 12 code words a frame each
    nine = iter(range(1024 + 400))
    for part in range(3):
        made = []
        for _ in range(2):
            cells = {(sb, 0): (3, 2, (3 * (sb - 11), 0, 0), [0] * 36) for sb in range(11, 30)}
            codes = {(g, sb, 0): next(nine) % 1024 for sb in range(11, 30) for g in range(12)}
            made.append(chosen(64, MONO, True, cells, codes=codes))
        add("every code of class 9, part %d" % part, 64, True, made)
    made, five, three = [], iter(range(10 ** 6)), iter(range(10 ** 6))
    for _ in range(2):
        cells = {(sb, 0): (2 if sb < 21 else 1, sb % 4, (sb, 2 * sb, 62 - sb), [0] * 36) for sb in range(11, 30)}
        codes = {(g, sb, 0): next(five) % 128 if sb < 21 else next(three) % 32 for sb in range(11, 30) for g in range(12)}
        made.append(chosen(64, MONO, True, cells, codes=codes))
    add("every code of classes 5 and 3", 64, True, made)
    # ---- values: every code of the classes 7 .. 255 (the all-ones code is one of them).  48 kHz stereo, the large table:
    # sub-bands 0-2 hold 7, 15, .. 255 at a = 2 .. 7, sub-bands 3-10 hold 7 at a = 3
    made = []
    for k in range(4):
        cells = {(0, 0): (7, 0, (0, 1, 2), ramp(255, 72 * k)), (0, 1): (7, 1, (5, 0, 9), ramp(255, 72 * k + 36)),
                 (1, 0): (6, 2, (17, 0, 0), ramp(127, 36 * k)), (1, 1): (5, 3, (20, 31, 0), ramp(63, 36 * k)),
                 (2, 0): (4, 0, (40, 41, 45), ramp(31, 36 * k)), (2, 1): (3, 1, (60, 0, 62), ramp(15, 36 * k)),
                 (3, 0): (3, 2, (7, 0, 0), ramp(7, 36 * k))}
        made.append(chosen(192, STEREO, False, cells))
    add("every code of the classes 7 to 255", 192, False, made)
    # ---- values: both ends, the middle and the all-ones code of every larger class
    made = []
    for k in range(4):
        cells = {}
        for j, a in enumerate((8, 9, 10, 11, 12, 13, 14, 15)[4 * (k % 2):4 * (k % 2) + 4]):      # 511 .. 4095 | 8191 .. 65535
            n = 2 ** (a + 1) - 1
            cells[(j % 3, j // 3)] = (a, (j + k) % 4, (3 * j, 3 * j + 20, 3 * j + 40), ([0, n - 1, n, n // 2, 1, n - 2] * 6)[k:] + [n] * k)
        for j, a in enumerate((10, 11, 12, 13, 14, 15)):                                         # sub-bands 3-10: 511 .. 8191, 65535
            n = 65535 if a == 15 else 2 ** (a - 1) - 1
            cells[(3 + j, k % 2)] = (a, j % 4, (j, 30 + j, 50 - j), [n, 0, n - 1, n // 2 + 1, 2, n - 3] * 6)
        made.append(chosen(320, STEREO, False, cells))
    add("the ends and the all-ones code of the classes 511 to 65535", 320, False, made)
    # ---- all 63 scale-factor indices and the forbidden one; SCFSI 0 .. 3 with a different index in each part
    made = []
    for k in range(4):
        idx = iter(range(10 ** 6))
        cells = {(sb, ch): (1, 0, tuple((next(idx) + 16 * k) % 64 for _ in range(3)), [(sb + ch + t) % 3 for t in range(36)])
                 for sb in range(11) for ch in range(2)}
        for j, si in enumerate(range(4)):
            cells[(11 + j, k % 2)] = (2, si, (10 + j, 25 + k, 44 - j), [(t + j) % 5 for t in range(36)])
        made.append(chosen(128, STEREO, False, cells))
    add("every scale-factor index and every SCFSI", 128, False, made)
    # ---- shapes: every legal (rate, mode, ID), random frames; joint stereo with each mode extension
    for lsf, rates in ((False, synth.MP2_RATES_48K[1:]), (True, synth.MP2_RATES_24K[1:])):
        for B in rates:
            for mode in range(4):
                if legal(B, mode, lsf):
                    ext = int(rng.integers(4))
                    add("%d kbit/s mode %d ext %d %s" % (B, mode, ext, "24 kHz" if lsf else "48 kHz"), B, lsf,
                        [synth.mp2_audio_frame(rng, B, mode, ext, lsf) for _ in range(2 if lsf else 4)])
    for lsf, B in ((False, 128), (True, 96)):
        for ext in range(4):
            add("joint stereo bound %d %s" % (4 * ext + 4, "24 kHz" if lsf else "48 kHz"), B, lsf,
                [synth.mp2_audio_frame(rng, B, JOINT, ext, lsf, silent_bands=0.1) for _ in range(2 if lsf else 4)])
    # ---- levels: silence by allocation, silence by the forbidden index, a PAD behind the audio
    label = synth.dls_pads(synth.dls_segments(b"layer two", toggle=1), length_index=3)
    quiet = chosen(64, STEREO, False, {})
    mute = chosen(64, STEREO, False, {(sb, ch): (2, 2, (63, 0, 0), [1] * 36) for sb in range(5) for ch in range(2)})
    add("silent frames and frames with a PAD", 64, False,
        [quiet, mute, synth.mp2_audio_frame(rng, 64, STEREO, pad=label[0]), synth.mp2_audio_frame(rng, 64, STEREO, pad=label[1])])
    # ---- failures.  Slots that are not GOOD: a damaged allocation, a damaged header, no CRC
    good = [synth.mp2_audio_frame(rng, 96, JOINT, 1) for _ in range(4)]
    lf = logical([f for f, _t in good], 96)
    lf = T.flip(T.flip(lf, 1, 48 + 3), 2, 5)
    lf[3, 1] |= 1
    add("slots that are not good", 96, False, good, lf=lf, kinds=[0, 1, 1, 1])
    # ... the end of the audio: exactly at 8 (L - 6 - c), and one bit behind it
    exact, over = frames_at_the_limit()
    add("the audio ends at the limit, and one bit behind it", 8, True, [exact, over], kinds=[0, 2])
    # ... a GOOD frame whose SCFSI, or whose scale factors, run behind the limit (the ISO CRC covers bits up to 8 L)
    full = {(sb, ch): (1, 2, (9, 0, 0), [1] * 36) for sb in range(30) for ch in range(2)}
    fewer = {cell: v for cell, v in full.items() if cell[0] < 25}
    short_scfsi, short_scf = chosen(8, STEREO, True, full, fit=False), chosen(8, STEREO, True, fewer, fit=False)
    assert 198 + 2 * 60 > 304 >= 198 + 2 * 50 and 198 + 2 * 50 + 6 * 50 > 304 and 198 + 2 * 60 <= 8 * 48
    add("the SCFSI and the scale factors run behind the limit", 8, True, [short_scfsi, short_scf], kinds=[2, 2])
    # ... a flipped sample bit: other values, the same kind
    clean = [synth.mp2_audio_frame(rng, 64, STEREO, silent_bands=0.0) for _ in range(4)]
    lf = logical([f for f, _t in clean], 64)
    add("unharmed", 64, False, clean)
    add("a flipped sample bit", 64, False, clean, lf=T.flip(lf, 2, A.decode(bytes(lf[2]), 64, 1)["E"] - 20), kinds=[0, 0, 0, 0])
    # ---- the carry: a 24 kHz frame whose first half the follow call held
    low = logical([f for f, _t in [synth.mp2_audio_frame(rng, 48, STEREO, 0, True) for _ in range(3)]], 48)
    add("24 kHz, the first half in the carry record", 48, True, None, carry=M.follow([low[0]], 48)["carry"], lf=low[1:5], kinds=[0, 0])
    add("24 kHz from a second half on", 48, True, None, lf=low[1:5], kinds=[0])
    return cases


def frames_at_the_limit():
    """two frames at 8 kbit/s and 24 kHz (L = 48, the audio ends in front of bit 304).  Joint stereo with bound 12 has
    48 + 75 + 39 = 162 bits in front of the SCFSI, and two cells of class 3 with one and two indices sent end the audio at
    162 + 4 + 18 + 12 * 10 = 304; with bound 4 it has 139, and a cell of class 3 and one of class 5 end it at
    139 + 4 + 18 + 12 * 12 = 305"""
    exact = chosen(8, JOINT, True, {(11, 0): (1, 2, (5, 0, 0), ramp(2, 0)), (11, 1): (1, 1, (6, 0, 9), ramp(2, 1))}, mode_ext=2)
    over = chosen(8, JOINT, True, {(0, 0): (1, 2, (5, 0, 0), ramp(2, 0)), (0, 1): (2, 1, (6, 0, 9), ramp(4, 1))}, mode_ext=0, fit=False)
    return exact, over


CASES = build_cases()


# ------------------------------------------------------------------------------------------------------------ memory
class Host(T.HostMemory):
    def chain(self, follow, audio, n_cifs):
        L = dabgpu.lib()
        rc = L.dabgpu_mp2_follow_host((dabgpu.Mp2Entry * max(len(follow), 1))(*follow), len(follow), n_cifs)
        return rc, L.dabgpu_mp2_subbands_host((dabgpu.Mp2AudioEntry * max(len(audio), 1))(*audio), len(audio), n_cifs)


class Device(T.DeviceMemory):
    def chain(self, follow, audio, n_cifs):
        """both calls on the context's stream, no host synchronisation between them"""
        rc = [None, None]
        try:
            self.ctx.mp2_follow_dev(follow, n_cifs)
            rc[0] = 0
            self.ctx.mp2_subbands_dev(audio, n_cifs)
            rc[1] = 0
        except dabgpu.DabGpuError as e:
            rc[rc.index(None)] = e.status
        self.ctx.sync()
        return tuple(rc)


class Arena:
    """every buffer of a call in one block of sentinel bytes: one copy up, one copy down"""
    def __init__(self):
        self.parts, self.size = [], 256

    def add(self, data, align=16, off=0):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        start = (self.size + align - 1) // align * align + off
        self.parts.append((start, data))
        self.size = start + len(data) + 16
        return start, len(data)

    def block(self):
        buf = np.full(self.size, SENTINEL, np.uint8)
        for start, data in self.parts:
            buf[start:start + len(data)] = data
        return buf


def run(mem, specs, n_cifs, mutate=None):
    """specs: dicts {B, frames [n_cifs][3 B], carry, pad (extra in_stride), in_off (d_in off its boundary), sub (False:
    d_subbands NULL)} -> ((rc of the follow call, rc of the audio call), [outputs per entry])"""
    arena, where = Arena(), []
    fill = lambda n: np.full(n, SENTINEL, np.uint8)
    for sp in specs:
        B, stride = sp["B"], 3 * sp["B"] + sp.get("pad", 0)
        src = np.full((max(n_cifs, 1), stride), 0x55, np.uint8)
        src[:n_cifs, :3 * B] = sp["frames"]
        w = dict(src=arena.add(src, off=sp.get("in_off", 0)))
        if sp.get("carry") is not None:
            w["cin"] = arena.add(np.frombuffer(sp["carry"], np.uint8))
        w["cout"] = arena.add(fill(M.carry_bytes(B)))
        w["rows"] = arena.add(fill((n_cifs + 1) * 220))
        w["status"] = arena.add(fill((n_cifs + 1) * 64))
        w["follow"] = arena.add(fill(32))
        w["result"] = arena.add(fill(64))
        w["levels"] = arena.add(fill((n_cifs + 2) * 32))
        if sp.get("sub", True):
            w["sub"] = arena.add(fill((n_cifs + 2) * FRAME_VALUES * 4))
        w["audio"] = arena.add(fill(32))
        where.append(w)
    before = arena.block()
    buf, base = mem.put(before, align=256)
    at = lambda w, k: base + w[k][0] if k in w else None
    follow = [dabgpu.Mp2Entry(at(w, "src"), 3 * sp["B"] + sp.get("pad", 0), sp["B"], at(w, "cin"), at(w, "cout"), at(w, "rows"),
                              at(w, "status"), at(w, "follow"), at(w, "result")) for sp, w in zip(specs, where)]
    audio = [dabgpu.Mp2AudioEntry(at(w, "src"), 3 * sp["B"] + sp.get("pad", 0), sp["B"], at(w, "cin"), at(w, "status"), at(w, "result"),
                                  at(w, "levels"), at(w, "sub"), at(w, "audio")) for sp, w in zip(specs, where)]
    if mutate:
        mutate(audio)
    rc = mem.chain(follow, audio, n_cifs)
    after = mem.get(buf)
    outs, written = [], np.zeros(len(after), bool)
    for w in where:
        cut = lambda k: after[w[k][0]:w[k][0] + w[k][1]]
        outs.append(dict(levels=cut("levels"), sub=cut("sub").view(np.float32).reshape(-1, 2, 36, 32) if "sub" in w else None,
                         audio=cut("audio"), result=cut("result").view(dabgpu.MP2_RESULT_DTYPE)[0], status=cut("status")))
        for k in ("cout", "rows", "status", "follow", "result", "levels", "sub", "audio"):
            if k in w:
                written[w[k][0]:w[k][0] + w[k][1]] = True
    assert (after[~written] == before[~written]).all(), "bytes outside the outputs were written"
    return rc, outs


def untouched(out):
    return all((out[k].view(np.uint8) == SENTINEL).all() for k in ("levels", "audio", "sub") if out[k] is not None)


def expected(sp):
    """what the reference makes of one entry (kept in the spec: the cases are shared)"""
    if "_want" not in sp:
        followed = M.follow(list(sp["frames"]), sp["B"], sp.get("carry"))
        sp["_want"] = (followed,) + A.subbands(list(sp["frames"]), sp["B"], sp.get("carry"), followed)
    return sp["_want"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(out, sp, what):
    """one entry's outputs against the reference's, and the sentinel bytes in the rows that are not written"""
    followed, rows, tally = expected(sp)
    n = len(rows)
    assert int(out["result"]["frames"]) == n, what
    levels = out["levels"][:32 * n].view(LEVEL)
    for k, (dec, lv) in enumerate(zip(rows, levels)):
        kind, channels, cells, scf63, power, peak = A.level(dec)
        assert (int(lv["kind"]), int(lv["channels"]), int(lv["cells"]), int(lv["scf63"])) == (kind, channels, cells, scf63), (what, k)
        assert (bits(lv["peak"]) == bits(peak)).all(), (what, k, lv["peak"], peak)
        assert (np.abs(lv["power"].astype(np.float64) - power) <= POWER_TOL * power).all(), (what, k, lv["power"], power)
        if out["sub"] is not None:
            assert (bits(out["sub"][k]) == bits(dec["v32"])).all(), (what, k)
        if kind != A.DECODED:
            assert lv.tobytes()[4:] == bytes(28), (what, k)
    assert (out["levels"][32 * n:] == SENTINEL).all(), what
    if out["sub"] is not None:
        assert (out["sub"][n:].view(np.uint8) == SENTINEL).all(), what
    assert out["audio"].view(np.int32).tolist() == tally + [0, 0, 0, 0], (what, out["audio"].view(np.int32), tally)
    assert sum(tally[:3]) == n
    return rows, tally


def check_case(name, out):
    c = CASES[name]
    rows, tally = compare(out, c, name)
    if c["kinds"] is not None:
        assert [r["kind"] for r in rows] == c["kinds"], name
    if c["truth"] is not None and c["kinds"] is None:
        assert len(rows) == len(c["truth"]) and tally[0] == len(rows), name
        for k, (dec, truth) in enumerate(zip(rows, c["truth"])):
            err = np.abs(out["sub"][k].astype(np.float64) - truth)
            assert (err <= VALUE_TOL * np.abs(truth)).all(), (name, k, (err[truth != 0] / np.abs(truth[truth != 0])).max() / U)
            assert (dec["v64"] == truth).all(), (name, k)                  # (reference and generator: one definition)
            if dec["channels"] == 1:
                assert (out["sub"][k][1] == 0).all() and out["levels"][32 * k:32 * k + 32].view(LEVEL)[0]["power"][1] == 0, name


# ---- the table block: a frame with one active cell for every (table, sub-band, allocation index)
TABLES = {"48 kHz large": (56, False, A.LEVELS_48K_LARGE), "48 kHz small": (32, False, A.LEVELS_48K_SMALL),
          "24 kHz": (16, True, A.LEVELS_24K)}


def table_specs(which):
    B, lsf, table = TABLES[which]
    specs = []
    for sb, row in enumerate(table):
        for a, n in enumerate(row, 1):
            # scale-factor index 3 is the factor 1; the first sample makes 2 s + 1 - n = 2, so the value is 2 R[n]
            f, _t = chosen(B, MONO, lsf, {(sb, 0): (a, 2, (3, 0, 0), [(n + 1) // 2] + [(7 * t) % n for t in range(35)])})
            specs.append(dict(B=B, frames=f.reshape(-1, 3 * B), sb=sb, n=n))
    return specs


TABLE_SPECS = {which: table_specs(which) for which in TABLES}


def check_table_block(mem, which):
    specs = TABLE_SPECS[which]
    rc, outs = run(mem, specs, 2 if TABLES[which][1] else 1)
    assert rc == (0, 0) and len(specs) == sum(len(r) for r in TABLES[which][2])
    for sp, out in zip(specs, outs):
        rows, _t = compare(out, sp, (which, sp["sb"], sp["n"]))
        assert len(rows) == 1 and rows[0]["classes"] == {(sp["sb"], 0): sp["n"]}
        assert round(2.0 / float(out["sub"][0][0][0][sp["sb"]])) == sp["n"], (which, sp["sb"], sp["n"])


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_are_exported_and_typed(built):
    L = dabgpu.lib()
    for name in ("dabgpu_mp2_subbands_dev", "dabgpu_mp2_subbands_host"):
        assert name in dabgpu.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.dabgpu_abi_version() == 6 == dabgpu.ABI_VERSION
    assert C.sizeof(dabgpu.Mp2AudioEntry) == 72 and LEVEL.itemsize == 32 and RESULT.itemsize == 32
    assert dabgpu.MP2_SUBBANDS_SHAPE == (2, 36, 32)
    assert (dabgpu.MP2_AUDIO_DECODED, dabgpu.MP2_AUDIO_NOT_GOOD, dabgpu.MP2_AUDIO_OVERRUN) == (A.DECODED, A.NOT_GOOD, A.OVERRUN)
    assert hasattr(dabgpu.Context, "mp2_subbands_dev") and hasattr(dabgpu, "mp2_subbands_host")
    assert hasattr(synth, "mp2_audio_frame") and hasattr(synth, "mp2_audio_pack")


def test_binding_matches_the_header(tmp_path):
    fields = [f for f, _ in dabgpu.Mp2AudioEntry._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dabgpu.h"', 'int main(void) {',
             '  printf("%zu", sizeof(dabgpu_mp2_audio_entry));']
    lines += ['  printf(" %%zu", offsetof(dabgpu_mp2_audio_entry, %s));' % f for f in fields]
    lines += ['  printf("\\n%zu", sizeof(dabgpu_mp2_level));']
    lines += ['  printf(" %%zu", offsetof(dabgpu_mp2_level, %s));' % f for f in LEVEL.names]
    lines += ['  printf("\\n%zu", sizeof(dabgpu_mp2_audio_result));']
    lines += ['  printf(" %%zu", offsetof(dabgpu_mp2_audio_result, %s));' % f for f in RESULT.names]
    lines += ['  return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(tmp_path / "layout")])
    entry, level, result = [[int(v) for v in line.split()] for line in subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")]
    assert entry == [C.sizeof(dabgpu.Mp2AudioEntry)] + [getattr(dabgpu.Mp2AudioEntry, f).offset for f in fields]
    assert level == [32] + [LEVEL.fields[f][1] for f in LEVEL.names]
    assert result == [32] + [RESULT.fields[f][1] for f in RESULT.names]


def test_the_generator_leaves_the_old_draws_alone_and_fits_its_audio():
    """synth.mp2_frame draws what it drew; mp2_audio_frame's frames are GOOD for the follow reference and end in front of
    L - 6 - c, PAD included"""
    import zlib
    assert zlib.crc32(synth.mp2_frame(np.random.default_rng(3), 64).tobytes()) == 3645230640           # (as before this call existed)
    assert zlib.crc32(synth.mp2_frame(np.random.default_rng(4), 48, mode=1, mode_ext=2, lsf=True).tobytes()) == 1153765904
    for name, c in CASES.items():
        if c["truth"] is not None and c["kinds"] is None:
            _f, rows, tally = expected(c)
            assert tally[0] == len(rows) and all(r["E"] <= r["limit"] for r in rows), name


@pytest.mark.parametrize("which", list(TABLES))
def test_table_block_on_the_host(built, which):
    check_table_block(Host(), which)


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_reference_and_the_truth(built, name):
    rc, (out,) = run(Host(), [dict(CASES[name], pad=len(name) % 5)], 4)
    assert rc == (0, 0)
    check_case(name, out)


def test_the_cases_are_what_they_say(built):
    """the exhaustive cases do cover what their names promise (read from the reference's view of them)"""
    wide = set()
    for c in CASES.values():
        for dec in expected(c)[1]:
            wide |= {n for n in dec["classes"].values() if n > 255}
    assert wide == {511, 1023, 2047, 4095, 8191, 16383, 32767, 65535}
    # the forbidden index is counted where it is sent, and makes its part silent
    _f, rows, tally = expected(CASES["every scale-factor index and every SCFSI"])
    assert all(r["scf63"] >= 1 for r in rows)
    _f, rows, tally = expected(CASES["silent frames and frames with a PAD"])
    assert tally == [4, 0, 0, 2] and rows[1]["scf63"] == 10 and rows[1]["cells"] == 10 and rows[0]["cells"] == 0
    _f, rows, tally = expected(CASES["the audio ends at the limit, and one bit behind it"])
    assert rows[0]["E"] == rows[0]["limit"] == 304 and rows[1]["E"] == 305 and tally == [1, 0, 1, 0]
    _f, rows, tally = expected(CASES["the SCFSI and the scale factors run behind the limit"])
    assert [r["E"] for r in rows] == [None, None] and tally == [0, 0, 2, 0]
    a, b = (expected(CASES[n])[1] for n in ("unharmed", "a flipped sample bit"))
    assert 1 <= (a[2]["v32"] != b[2]["v32"]).sum() <= 3 and all((x["v32"] == y["v32"]).all() for x, y in zip(a[:2] + a[3:], b[:2] + b[3:]))
    _f, rows, tally = expected(CASES["24 kHz, the first half in the carry record"])
    assert tally[0] == 2
    _f, rows, tally = expected(CASES["24 kHz from a second half on"])
    assert tally[0] == 1


def test_every_grouped_code_is_sent(built):
    """the code words of the grouped cases, read back by the reference's own bit reader: all 1024, 128 and 32"""
    got = {3: set(), 5: set(), 9: set()}
    for name, c in CASES.items():
        if not name.startswith("every code of class"):
            continue
        for k in range(2):
            frame = bytes(c["frames"][2 * k]) + bytes(c["frames"][2 * k + 1])
            dec = A.decode(frame, c["B"], 0)
            b = M.bits_of(frame)
            at = dec["E"] - 12 * sum(A.GROUPED[n] for n in dec["classes"].values())
            for _g in range(12):
                for cell in sorted(dec["classes"]):
                    n = dec["classes"][cell]
                    got[n].add(M.number(b[at:at + A.GROUPED[n]]))
                    at += A.GROUPED[n]
    assert got[9] == set(range(1024)) and got[5] == set(range(128)) and got[3] == set(range(32))


def _entry(bitrate=64, d_in=0x10000, stride=None, cin=0x20000, status=0x30000, result=0x40000, levels=0x50000, sub=0x60000, audio=0x70000):
    return dabgpu.Mp2AudioEntry(d_in, 3 * bitrate if stride is None else stride, bitrate, cin, status, result, levels, sub, audio)


_set = T._set
BAD_ENTRIES = [
    ("bit rate no multiple of 8", _set(1, bitrate_kbps=68)),
    ("bit rate 0", _set(0, bitrate_kbps=0)),
    ("bit rate negative", _set(0, bitrate_kbps=-64)),
    ("bit rate above 384", _set(1, bitrate_kbps=392, in_stride=4096)),
    ("in_stride below bitrate * 3", _set(1, in_stride=lambda v: 191)),
    ("carry in off its boundary", _set(0, d_carry_in=lambda v: (v or 0x1000) + 8)),
    ("null input", _set(1, d_in=None)),
    ("null status", _set(1, d_status=None)),
    ("null result", _set(0, d_result=None)),
    ("null levels", _set(1, d_levels=None)),
    ("null audio", _set(0, d_audio=None)),
    ("status off its boundary", _set(1, d_status=lambda v: v + 2)),
    ("result off its boundary", _set(0, d_result=lambda v: v + 1)),
    ("levels off their boundary", _set(1, d_levels=lambda v: v + 2)),
    ("audio off its boundary", _set(0, d_audio=lambda v: v + 3)),
    ("sub-bands off their boundary", _set(1, d_subbands=lambda v: v + 8)),
]


def refusal_specs():
    return [dict(CASES["unharmed"]), dict(CASES["a flipped sample bit"], pad=3)]


def check_refusals(mem):
    for what, m in BAD_ENTRIES:
        rc, outs = run(mem, refusal_specs(), 4, mutate=m)
        assert rc == (0, ARG), what
        assert all(untouched(o) for o in outs), what                 # the good entry in front of the bad one too
    rc, outs = run(mem, refusal_specs(), 4)
    assert rc == (0, 0) and not any(untouched(o) for o in outs)


def test_refusals_of_the_host_twin(built):
    check_refusals(Host())
    L = dabgpu.lib()
    good = (dabgpu.Mp2AudioEntry * 1)(_entry())
    assert L.dabgpu_mp2_subbands_host(None, 1, 4) == ARG
    assert L.dabgpu_mp2_subbands_host(good, -1, 4) == ARG
    assert L.dabgpu_mp2_subbands_host(good, 1, -1) == ARG
    assert L.dabgpu_mp2_subbands_host(good, 1, (1 << 28) + 1) == ARG
    assert L.dabgpu_mp2_subbands_dev(None, good, 1, (1 << 28) + 1, None) == ARG
    assert L.dabgpu_mp2_subbands_host(None, 0, 4) == 0                   # nothing to do is not an error
    assert L.dabgpu_mp2_subbands_dev(None, good, 1, 4, None) == ARG      # no context
    # d_in may be NULL with n_cifs = 0, d_subbands may be NULL: the record is written, no row is
    rc, (out,) = run(Host(), [dict(B=64, frames=np.zeros((0, 192), np.uint8), sub=False)], 0, mutate=_set(0, d_in=None))
    assert rc == (0, 0) and out["audio"].view(np.int32).tolist() == [0] * 8 and (out["levels"] == SENTINEL).all()


def test_audio_fuzz_under_sanitizers(tmp_path):
    """tests/mp2_audio_fuzz.cpp: 60 000 random and mutated frames with a repaired ISO CRC at every rate through the serial
    decoder, every logical frame in an exactly sized heap block behind a callable that aborts on an index outside [0, L),
    built with the host compiler under AddressSanitizer and UBSan and run as a child process"""
    exe = str(tmp_path / "mp2_audio_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mp2_audio_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "60000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "frames=60000" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
    assert got["decoded"] + got["overrun"] == got["good"] and min(got["decoded"], got["overrun"], got["scf63"]) > 1000, r.stdout


def test_kernels_use_no_scratch_and_spill_nothing(built, tmp_path):
    """the metadata of mp2_audio_kernels.o, the object the library is linked from: two kernels, no scratch, no spills"""
    obj = os.path.join(CSRC, "mp2_audio_kernels.o")
    llvm = "/opt/rocm/lib/llvm/bin/"
    if not (os.path.exists(obj) and os.path.exists(llvm + "llvm-readelf")):
        pytest.fail("toolchain or mp2_audio_kernels.o missing")
    fat, co = str(tmp_path / "mp2a.fat"), str(tmp_path / "mp2a.co")
    subprocess.check_call([llvm + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([llvm + "clang-offload-bundler", "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    md = kernel_metadata(subprocess.check_output([llvm + "llvm-readelf", "--notes", co], text=True))
    assert len(md) == 2 and any("mp2_audio_kernel" in k for k in md) and any("mp2_audio_zero_kernel" in k for k in md), list(md)
    for k, v in md.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_count"] <= 128 and v.get("agpr_count", 0) == 0, (k, v)


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def actx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.gpu
def test_gpu_every_case_in_one_call(actx):
    names = list(CASES)
    rc, outs = run(Device(actx), [dict(CASES[n], pad=[0, 8, 3][j % 3]) for j, n in enumerate(names)], 4)
    assert rc == (0, 0)
    for name, out in zip(names, outs):
        check_case(name, out)


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(TABLES))
def test_gpu_table_block(actx, which):
    check_table_block(Device(actx), which)


@pytest.fixture(scope="module")
def seam_frames():
    """frames for the seams of the wave-per-frame layout, every field active where the name says so"""
    rng = np.random.default_rng(0x5EA2)
    make = lambda n, B, mode, lsf, **kw: logical([synth.mp2_audio_frame(rng, B, mode, 0, lsf, **kw)[0] for _ in range(n)], B)
    return dict(lanes60=make(3, 160, STEREO, True, silent_bands=0.0), lanes30=make(3, 160, MONO, True, silent_bands=0.0),
                lanes8=make(6, 32, MONO, False, silent_bands=0.0), sblimit27=make(6, 384, STEREO, False, silent_bands=0.0),
                smallest=make(3, 8, DUAL, True, silent_bands=0.5), run=make(12, 96, JOINT, False))


def wide_field_starts(frame, B, id_):
    """bit positions (mod 32) at which the 48-bit fields of a frame's 16-bit cells begin, from the reference's layout"""
    dec = A.decode(bytes(frame), B, id_)
    h = M.header(frame, B)
    channels, nbal, bound, _c = M.shape(h, B)
    fields = [(sb, ch) for sb in range(len(nbal)) for ch in range(1 if channels == 2 and sb >= bound else channels) if (sb, ch) in dec["classes"]]
    width = lambda n: A.GROUPED[n] if n in A.GROUPED else 3 * A.SAMPLE_BITS[n]
    at, starts = dec["E"] - 12 * sum(width(dec["classes"][f]) for f in fields), set()
    for _g in range(12):
        for f in fields:
            if dec["classes"][f] == 65535:
                starts.add(at % 32)
            at += width(dec["classes"][f])
    return starts


@pytest.mark.gpu
def test_gpu_seams_of_the_wave_per_frame_layout(actx, seam_frames):
    """busy lanes: 60 (24 kHz two-channel), 30 (24 kHz single channel), 8 (the small table), 54 (sblimit 27); the largest
    frame (384 kbit/s, 1152 bytes) and the smallest (8 kbit/s at 24 kHz, 48 bytes); frames off their 16-byte and their
    4-byte boundary; sub-bands wanted and not wanted in one call; 48-bit fields over two and over three 32-bit words"""
    s = seam_frames
    specs = [dict(B=160, frames=s["lanes60"]), dict(B=160, frames=s["lanes30"], pad=1, in_off=1),
             dict(B=32, frames=s["lanes8"], sub=False), dict(B=32, frames=s["lanes8"], in_off=4),
             dict(B=384, frames=s["sblimit27"], in_off=8), dict(B=384, frames=s["sblimit27"], pad=3, in_off=3, sub=False),
             dict(B=8, frames=s["smallest"]), dict(B=8, frames=s["smallest"], pad=5, in_off=2),
             dict(B=96, frames=s["run"][:6], pad=8, sub=False), dict(B=96, frames=s["run"][3:9], pad=7, in_off=13)]
    rc, outs = run(Device(actx), specs, 6)
    assert rc == (0, 0)
    cells = []
    for k, (sp, out) in enumerate(zip(specs, outs)):
        rows, tally = compare(out, sp, k)
        assert tally[0] == len(rows) == (3 if sp["B"] in (160, 8) else 6), k
        cells.append(rows[0]["cells"])
    assert cells[0] == 60 and cells[1] == 30 and cells[2] == cells[3] == 8 and cells[4] == 54
    starts = set()
    for f in CASES["the ends and the all-ones code of the classes 511 to 65535"]["frames"]:
        starts |= wide_field_starts(f, 320, 1)
    assert any(p <= 16 for p in starts) and any(p > 16 for p in starts)      # (48 bits from p: two words | three)
    host = run(Host(), specs, 6)[1]
    for g, h in zip(outs, host):
        assert all(g[k].tobytes() == h[k].tobytes() for k in ("status", "audio")) and (g["sub"] is None or bits(g["sub"]).tobytes() == bits(h["sub"]).tobytes())
        a, b = g["levels"].view(LEVEL)[:6], h["levels"].view(LEVEL)[:6]
        assert all(a[f].tobytes() == b[f].tobytes() for f in ("kind", "channels", "cells", "scf63", "peak"))


@pytest.mark.gpu
@pytest.mark.parametrize("n_cifs", [0, 3, 4, 5, 9])
def test_gpu_row_counts_around_a_workgroup(actx, seam_frames, n_cifs):
    """a workgroup decodes four frames: rows one less than, exactly and one more than that, at 48 kHz, behind a held frame
    (one row more) and at 24 kHz behind a held half; n_cifs = 0 with a held half (no row) and with a held frame (one row)"""
    r48, r24 = seam_frames["run"], seam_frames["lanes60"]
    held48 = T.struct_carry(0, 1, 0, r48[0])
    held24 = M.follow([r24[0]], 160)["carry"]
    specs = [dict(B=96, frames=r48[:n_cifs]), dict(B=96, frames=r48[1:1 + n_cifs], carry=held48, pad=8),
             dict(B=160, frames=np.concatenate([r24, r24])[1:1 + n_cifs], carry=held24),
             dict(B=96, frames=r48[:n_cifs], sub=False, in_off=1)]
    rc, outs = run(Device(actx), specs, n_cifs)
    assert rc == (0, 0)
    rows = [len(compare(out, sp, (n_cifs, k))[0]) for k, (sp, out) in enumerate(zip(specs, outs))]
    assert rows == [n_cifs, n_cifs + 1, (n_cifs + 1) // 2, n_cifs]


@pytest.mark.gpu
def test_gpu_forty_entries_of_mixed_rates_behind_the_follow_call(actx):
    """40 entries in ONE call of each kind, the audio call enqueued behind the follow call on one stream with no host
    synchronisation between them: every 48 kHz rate, every 24 kHz rate, modes in rotation, odd strides, frames off their
    boundaries, some with a held half, some damaged, some silent, every third without sub-bands -- each against the
    reference fed from the follow reference's rows"""
    rng = np.random.default_rng(41)
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
        frames = logical([synth.mp2_audio_frame(rng, B, mode, k % 4, lsf)[0] for _ in range(6 if lsf else 12)], B)
        sp = dict(B=B, pad=[0, 8, 3, 16][k % 4], in_off=[0, 1, 4, 0, 6][k % 5], sub=k % 3 != 2)
        if lsf and k % 2:
            sp["carry"], frames = M.follow([frames[0]], B)["carry"], frames[1:]
        if k % 7 == 3:
            frames = T.flip(frames, 4, 48 + k)
        if k == 20:
            frames = np.zeros_like(frames)
        sp["frames"] = frames[:n_cifs]
        specs.append(sp)
    rc, outs = run(Device(actx), specs, n_cifs)
    assert rc == (0, 0)
    total = np.zeros(4, np.int64)
    for k, (sp, out) in enumerate(zip(specs, outs)):
        total += compare(out, sp, k)[1]
    assert total[0] > 250 and total[1] >= 5 and total[2] == 0


@pytest.mark.gpu
def test_gpu_refused_calls_leave_every_output_alone(actx):
    check_refusals(Device(actx))
    with pytest.raises(dabgpu.DabGpuError):
        actx.mp2_subbands_dev([dabgpu.Mp2AudioEntry()], 4)
    actx.mp2_subbands_dev([], 4)                                         # nothing to do is not an error
