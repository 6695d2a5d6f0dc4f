"""dabgpu_dabplus_follow_dev and dabgpu_eti_frames_dev at the call lengths the library runs them at: every loop whose trip
count a call argument sets, taken through its second trip and a ragged last one (the census: tests/README.md and CENSUS
below).  Bit for bit against tests/dabplus_follow_reference.py and tests/eti_reference.py, through the helpers of
test_dabplus_follow.py (call: the whole allocation, sentinels included) and test_eti.py (check_against_reference: every byte
of every frame, every status field, the history record).

CPU: the census' assertions, the mutant study of the follow reference on the GPU tests' own inputs, what the decoy headers
would do if they were counted, the ETI sweep's coverage of the data CRC's (chunk_words, lead) and the largest frames."""
import functools
import os
import re

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import dabplus_follow_reference as F
import eti_reference as R
from conftest import ROOT, make_ctx
from test_dabplus_follow import call, damage_columns, decoy_count, held_of
from test_eti import CONFIGS, check_against_reference, make_case, run_eti, service_chain  # noqa: F401 (service_chain: a fixture)

CSRC = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")


# =================================================================================================== follow: the inputs
@functools.lru_cache(maxsize=None)
def long_stream(s):
    """29 clean super-frames (145 logical frames) -> (frames, the transmitted super-frames)"""
    frames, sfs, _starts = F.build_stream(900, 8 * s, 29)
    return frames, sfs


def carry_of(s, frames, synced):
    """the carry record that holds `frames` (0..4 logical frames)"""
    frames = np.asarray(frames, np.uint8).reshape(-1, 24 * s)
    c = np.zeros(F.carry_bytes(s), np.uint8)
    c[:16].view("<i4")[:2] = [synced, len(frames)]
    c[16:16 + frames.size] = frames.reshape(-1)
    return c


def sequence_of(sp):
    """the frames the entry's call votes over: the carry's held frames, then the new ones"""
    s, held = sp["s"], held_of(sp)
    new = np.asarray(sp["frames"], np.uint8).reshape(-1, 24 * s)
    if not held:
        return new
    return np.concatenate([np.asarray(sp["carry"][16:16 + held * 24 * s], np.uint8).reshape(held, 24 * s), new])


def decoy():
    """eleven bytes that pass the raw check: a transmitted super-frame's own header"""
    return long_stream(8)[0][0, :11].copy()


BOUNDARY_CIFS = [59, 60, 63, 64, 65, 69, 124, 128, 129, 133]
GEOMETRY = [(0, 0), (8, 8), (5, 1), (16, 16), (0, 3)]           # (in_stride - 24 s, the input's bytes off its 256-byte boundary)


@functools.lru_cache(maxsize=None)
def boundary_specs(n_cifs):
    """s = 1 and 8, a carry of 0..4 held frames each: T = held + n_cifs lands on every side of 64 and 128.  The sequence begins
    `off` frames into the stream, so its phase is -off mod 5; every other carry says synced (rightly only where off = 0: the
    others are outvoted by a dozen hits).  Decoy headers behind every entry's last frame."""
    specs = []
    for s in (1, 8):
        frames, _sfs = long_stream(s)
        for held in range(5):
            off = (3 * held + n_cifs + s) % 5
            seq = frames[off:off + held + n_cifs]
            pad, shift = GEOMETRY[(held + s) % 5]
            specs.append(dict(s=s, frames=seq[held:], carry=carry_of(s, seq[:held], (held + n_cifs) % 2) if held else None,
                              decoy=decoy(), stride=24 * s + pad, shift=shift, phase=-off % 5))
    return specs


LATER_CIFS = 84


@functools.lru_cache(maxsize=None)
def later_block_specs():
    """64 + ph erasure frames, then three super-frames: every raw hit lies at i >= 64, at each of the five phases.  A fresh
    start, a synced carry without frames and a synced carry of two erasure frames (which moves every hit by two)."""
    specs = []
    for s in (1, 8):
        for ph in range(5):
            frames, _sfs, starts = F.build_stream(910 + ph, 8 * s, 3, lead=64 + ph)
            assert starts[0] == 64 + ph
            frames = np.concatenate([frames, F.erasure_frames(LATER_CIFS - len(frames), s)])
            specs.append(dict(s=s, frames=frames, carry=None, phase=(64 + ph) % 5))
            specs.append(dict(s=s, frames=frames, carry=carry_of(s, [], 1), phase=(64 + ph) % 5, decoy=decoy()))
            specs.append(dict(s=s, frames=frames, carry=carry_of(s, F.erasure_frames(2, s), 1), phase=(66 + ph) % 5, stride=24 * s + 8))
    return specs


TIE_CIFS = 75


def _placed(s, n, hits):
    """n erasure frames with one and the same super-frame (one raw hit, at its first frame) at every index of `hits`"""
    one, _sfs, _st = F.build_stream(920, 8 * s, 1)
    frames = F.erasure_frames(n, s).copy()
    for i in hits:
        frames[i:i + 5] = one
    return frames


@functools.lru_cache(maxsize=None)
def tie_specs():
    """[0, 1] one vote each for two residues, one in block 0 and one in block 1, the smaller residue in block 1 / in block 0;
    [2] a synced carry with one vote for residue 0, and two for residue 2 of which one lies in block 1; (per s = 8, then 1)"""
    specs = []
    for s in (8, 1):
        specs.append(dict(s=s, frames=_placed(s, TIE_CIFS, (3, 66)), carry=None, phase=1))
        specs.append(dict(s=s, frames=_placed(s, TIE_CIFS, (2, 68)), carry=None, phase=2))
        specs.append(dict(s=s, frames=_placed(s, TIE_CIFS, (0, 7, 67)), carry=carry_of(s, [], 1), phase=2))
    return specs


MANY_CIFS, MANY_DAMAGED = 133, {14: 3, 25: 5}                   # emitted super-frame -> byte errors in each of its columns


@functools.lru_cache(maxsize=None)
def many_superframes_specs():
    """133 CIFs behind a synced carry of two frames: 27 super-frames, two of them beyond index 12 with byte errors"""
    specs = []
    for s in (1, 8):
        frames, sfs = long_stream(s)
        seq = frames[:135].copy()
        rng = np.random.default_rng(930 + s)
        for k, n_errors in MANY_DAMAGED.items():
            sf = seq[5 * k:5 * k + 5].reshape(-1)
            damage_columns(sf, s, rng, n_errors)
            seq[5 * k:5 * k + 5] = sf.reshape(5, 24 * s)
        specs.append(dict(s=s, frames=seq[2:], carry=carry_of(s, seq[:2], 1), phase=0, stride=24 * s + (16 if s == 8 else 0), decoy=decoy()))
    return specs


BIG_S = [25, 32, 37, 38, 47, 48, 63, 64]
BIG_GEOMETRY = [(0, 0), (16, 1), (5, 8), (0, 16)]


@functools.lru_cache(maxsize=None)
def big_s_specs(s):
    """three super-frames cut at an offset (and as many erasure frames behind them: 15 frames for every entry), tight and
    padded strides, the input 0 / 1 / 8 / 16 bytes off its boundary -> (specs, what must come out)"""
    specs, want = [], []
    for g, (pad, shift) in enumerate(BIG_GEOMETRY):
        off = (g + s) % 5
        frames, sfs, _starts = F.build_stream(900, 8 * s, 3, cut_frames=off)
        specs.append(dict(s=s, frames=np.concatenate([frames, F.erasure_frames(off, s)]), carry=None, stride=24 * s + pad, shift=shift))
        want.append(sfs[1 if off else 0:, :110 * s])
    return specs, want


RAGGED_S = [1, 64, 3, 48, 24, 25]


@functools.lru_cache(maxsize=None)
def ragged_specs():
    specs = []
    for e, s in enumerate(RAGGED_S):
        off = 1 + e % 4
        frames, _sfs, _starts = F.build_stream(900, 8 * s, 3, cut_frames=off)
        pad, shift = GEOMETRY[e % 5]
        specs.append(dict(s=s, frames=np.concatenate([frames, F.erasure_frames(off, s)]), carry=None, stride=24 * s + pad, shift=shift,
                          decoy=decoy()))
    return specs


GROWTH_ENTRIES, GROWTH_CIFS = 200, 69


@functools.lru_cache(maxsize=None)
def growth_specs():
    """200 entries of s = 1, 2, 3 at their own phases; every third is all erasures"""
    streams = {s: F.build_stream(900, 8 * s, 15)[0] for s in (1, 2, 3)}
    specs = []
    for e in range(GROWTH_ENTRIES):
        s = 1 + (e // 2) % 3
        if e % 3 == 2:
            specs.append(dict(s=s, frames=F.erasure_frames(GROWTH_CIFS, s), carry=None, phase=-1))
        else:
            off = (e // 3) % 5
            specs.append(dict(s=s, frames=streams[s][off:off + GROWTH_CIFS], carry=None, phase=-off % 5, stride=24 * s + 8 * (e % 2)))
    return specs


@functools.lru_cache(maxsize=None)
def no_cifs_specs():
    """n_cifs = 0: the call has the carry alone, 0..4 held frames, with and without a start frame among them"""
    specs = []
    frames, _sfs = long_stream(8)
    for held in range(5):
        for a, synced in ((0, 1), (1, 0), (6 - held, 1)):
            specs.append(dict(s=8, frames=np.zeros((0, 192), np.uint8), carry=carry_of(8, frames[a:a + held], synced), decoy=decoy()))
    specs.append(dict(s=8, frames=np.zeros((0, 192), np.uint8), carry=None))
    return specs


def follow_inputs():
    """name -> (specs, n_cifs) of every call the GPU tests below make with fresh inputs (continued calls aside)"""
    inputs = {"boundary n_cifs=%d" % n: (boundary_specs(n), n) for n in BOUNDARY_CIFS}
    inputs["hits in later blocks"] = (later_block_specs(), LATER_CIFS)
    inputs["ties across blocks"] = (tie_specs(), TIE_CIFS)
    inputs["27 super-frames"] = (many_superframes_specs(), MANY_CIFS)
    for s in BIG_S:
        inputs["s=%d" % s] = (big_s_specs(s)[0], 15)
    inputs["ragged s"] = (ragged_specs(), 15)
    inputs["200 entries"] = (growth_specs(), GROWTH_CIFS)
    inputs["no CIFs"] = (no_cifs_specs(), 0)
    return inputs


# ======================================================================================= follow: the mutants, on the CPU
@functools.lru_cache(maxsize=None)
def _raw_hit(header):
    return F.raw_hit(np.frombuffer(header, np.uint8))


def raw_hits_of(seq):
    return [_raw_hit(bytes(bytearray(f[:11]))) for f in seq]


MUTANTS = {
    "lane residue": "the residue taken from the lane: (i % 64) % 5",
    "first block only": "votes from the first 64 frames only",
    "residue of the input": "the residue counted from the first new frame: (i - held) % 5",
    "tie to the larger": "a tie goes to the larger residue",
    "twelve super-frames": "n_superframes capped at 12",
    "synced margin": "the synced phase kept on votes[0] >= best - 1",
}


def decide(hits, synced, held, mutant=None):
    """F.follow's decisions from the frames' raw hits alone -> (n_superframes, phase, synced, dropped, raw_hits, held), the
    result record's fields; `mutant`: one of MUTANTS."""
    T = len(hits)
    votes = [0] * 5
    for i in range(T):
        if mutant == "first block only" and i >= 64:
            break
        r = (i % 64) % 5 if mutant == "lane residue" else (i - held) % 5 if mutant == "residue of the input" else i % 5
        votes[r] += hits[i]
    best = max(votes)
    if synced and (votes[0] >= best - 1 if mutant == "synced margin" else votes[0] == best):
        p = 0
    elif best > 0:
        p = 4 - votes[::-1].index(best) if mutant == "tie to the larger" else votes.index(best)
    else:
        return 0, -1, 0, T - min(4, T), sum(votes), min(4, T)
    n_sf = (T - p) // 5
    if mutant == "twelve super-frames":
        n_sf = min(n_sf, 12)
    return n_sf, p, int(votes[p] > 0 or n_sf == 0), p, sum(votes), T - p - 5 * n_sf


def decisions(sp, mutant=None, extra=()):
    synced = 0
    if sp.get("carry") is not None:
        hdr = np.asarray(sp["carry"][:16], np.uint8).view("<i4")
        synced = int(0 <= int(hdr[1]) <= 4 and hdr[0] != 0)          # (a record of anything but 0..4 frames is a fresh start)
    return decide(raw_hits_of(sequence_of(sp)) + list(extra), synced, held_of(sp), mutant)


#: mutant -> the input (follow_inputs' name, entry) that must tell it from F.follow
REJECTED_BY = {
    "lane residue": ("hits in later blocks", 0),
    "first block only": ("ties across blocks", 0),
    "residue of the input": ("boundary n_cifs=64", 1),
    "tie to the larger": ("ties across blocks", 1),
    "twelve super-frames": ("27 super-frames", 1),
    "synced margin": ("ties across blocks", 2),
}


def test_decide_is_the_reference_on_every_new_input(built):
    """decide() with no mutant gives F.follow's result record, field by field, on every entry of every new GPU input -- and
    the phases are the ones the inputs were built for.  The mutants below are mutants of decide(), not of F.follow itself:
    what their rejection says about F.follow rests on this test, which must stay with them."""
    n = 0
    for name, (specs, n_cifs) in follow_inputs().items():
        for e, sp in enumerate(specs):
            res = F.follow(sp["frames"], sp["s"], sp.get("carry"))[2]
            got = decisions(sp)
            assert got == tuple(int(res[k]) for k in ("n_superframes", "phase", "synced", "dropped", "raw_hits", "held")), (name, e)
            if "phase" in sp:
                assert got[1] == sp["phase"], (name, e)
            assert len(sp["frames"]) == n_cifs
            n += 1
    assert n >= 380


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_follow_mutant_is_rejected_by_a_new_input(built, mutant):
    assert sorted(REJECTED_BY) == sorted(MUTANTS)
    name, e = REJECTED_BY[mutant]
    sp = follow_inputs()[name][0][e]
    assert decisions(sp, mutant) != decisions(sp), (mutant, name, e)
    # ... and it is the new inputs that do it: no input of T <= 64 without a carry frame tells the block mutants apart
    if mutant in ("lane residue", "first block only"):
        short = dict(sp, frames=sequence_of(sp)[:64], carry=None)
        assert decisions(short, mutant) == decisions(short)


def test_counted_decoys_would_change_the_raw_hits(built):
    """were the idle lanes of the last block to read on, every decoy would be a vote"""
    n = 0
    for name, (specs, n_cifs) in follow_inputs().items():
        for e, sp in enumerate(specs):
            if sp.get("decoy") is None:
                continue
            k = decoy_count(sp, n_cifs)
            assert k == -(len(sequence_of(sp))) % 64
            if k == 0:
                continue
            assert F.raw_hit(sp["decoy"])
            assert decisions(sp, extra=[True] * k)[4] == decisions(sp)[4] + k, (name, e)
            n += 1
    assert n >= 100
    ts = {len(sequence_of(sp)) for n_cifs in BOUNDARY_CIFS for sp in boundary_specs(n_cifs)}
    assert {63, 64, 65, 68, 69, 128, 129, 132, 133} <= ts and max(ts) == 137


# ============================================================================================================ follow: GPU
@pytest.fixture(scope="module")
def fctx(built):
    c = make_ctx()
    yield c
    c.close()


def call_chunks(ctx, specs, chunks):
    """every entry fed in calls of `chunks` frames, the carry records handed on -> per call, call()'s results"""
    carries = [sp.get("carry") for sp in specs]
    got, at = [], 0
    for n in chunks:
        r = call(ctx, [dict(sp, frames=sp["frames"][at:at + n], carry=c) for sp, c in zip(specs, carries)], n)
        carries = [x[3] for x in r]
        got.append(r)
        at += n
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n_cifs", BOUNDARY_CIFS)
def test_gpu_follow_block_boundaries(fctx, n_cifs):
    specs = boundary_specs(n_cifs)
    got = call(fctx, specs, n_cifs)                                # (byte for byte, decoys and sentinels included: call())
    for sp, (data, st, res, _c) in zip(specs, got):
        T = held_of(sp) + n_cifs
        assert (res["phase"], res["n_superframes"], res["synced"]) == (sp["phase"], (T - sp["phase"]) // 5, 1)
        assert res["raw_hits"] == len(range(sp["phase"], T, 5)) and st["firecode_ok"].all() and len(data) == res["n_superframes"]


@pytest.mark.gpu
def test_gpu_follow_hits_that_only_later_blocks_hold(fctx):
    specs = later_block_specs()
    got = call(fctx, specs, LATER_CIFS)
    for sp, (_d, st, res, _c) in zip(specs, got):
        assert (res["phase"], res["raw_hits"], res["synced"]) == (sp["phase"], 3, 1) and st["firecode_ok"].sum() >= 3
    specs = tie_specs()
    got = call(fctx, specs, TIE_CIFS)
    assert [int(r[2]["phase"]) for r in got] == [sp["phase"] for sp in specs] == [1, 2, 2] * 2
    assert [int(r[2]["raw_hits"]) for r in got] == [2, 2, 3] * 2


@pytest.mark.gpu
def test_gpu_follow_27_superframes_of_one_entry(fctx):
    specs = many_superframes_specs()
    got = call(fctx, specs, MANY_CIFS)
    for sp, (data, st, res, _c) in zip(specs, got):
        s = sp["s"]
        assert (res["n_superframes"], res["phase"], res["held"], res["raw_hits"]) == (27, 0, 0, 27)
        assert (data == long_stream(s)[1][:27, :110 * s]).all() and st["firecode_ok"].all()
        assert [int(x) for x in st["rs_corrected"]] == [s * MANY_DAMAGED.get(k, 0) for k in range(27)]


@pytest.mark.gpu
@pytest.mark.parametrize("s", BIG_S)
def test_gpu_follow_large_s(fctx, s):
    specs, want = big_s_specs(s)
    calls = call_chunks(fctx, specs, [7, 8])
    for e in range(len(specs)):
        data = np.concatenate([c[e][0] for c in calls])
        st = np.concatenate([c[e][1] for c in calls])
        assert data.shape == want[e].shape and (data == want[e]).all() and st["firecode_ok"].all() and not st["rs_corrected"].any()


@pytest.mark.gpu
def test_gpu_follow_ragged_s_in_one_call(fctx):
    specs = ragged_specs()
    a = call(fctx, specs, 15)
    b = call(fctx, specs[::-1], 15)
    for x, y in zip(a, b[::-1]):
        assert x[2].tobytes() == y[2].tobytes() and (x[0] == y[0]).all() and x[2]["n_superframes"] == 2 and x[1]["firecode_ok"].all()


@pytest.mark.gpu
def test_gpu_follow_table_growth_and_no_cifs(built):
    ctx = make_ctx()                                               # its table has never held an entry
    try:
        specs = growth_specs()
        one = call(ctx, specs[:1], GROWTH_CIFS)
        got = call(ctx, specs, GROWTH_CIFS)
        again = call(ctx, specs[:1], GROWTH_CIFS)
        assert one[0][2].tobytes() == got[0][2].tobytes() == again[0][2].tobytes() and (one[0][0] == again[0][0]).all()
        for e, (sp, (data, st, res, _c)) in enumerate(zip(specs, got)):
            if e % 3 == 2:
                assert (res["phase"], res["n_superframes"], res["raw_hits"], res["held"]) == (-1, 0, 0, 4)
            else:
                assert (res["phase"], res["n_superframes"]) == (sp["phase"], (GROWTH_CIFS - sp["phase"]) // 5) and st["firecode_ok"].all()
        none = call(ctx, no_cifs_specs(), 0)
        assert all(r[2]["n_superframes"] == 0 and len(r[0]) == 0 for r in none)
        assert {int(r[2]["held"]) for r in none} == {0, 1, 2, 3, 4} and {int(r[2]["phase"]) for r in none} >= {-1, 0, 1}
    finally:
        ctx.close()


# ==================================================================================================== ETI: the layouts
def fold_shape(plan):
    """(chunk_words, lead) of the data CRC's fold: 24 + data_bytes / 4 words in 64 chunks, zeros in front"""
    n_words = 24 + plan.data_bytes // 4
    chunk_words = -(-n_words // 64)
    return chunk_words, 64 * chunk_words - n_words


def sweep_streams(k):
    """one EEP 4-A sub-channel of 8 k kbit/s = 24 k bytes (k = 0: the FIC alone), its id and place changing with k"""
    return [((7 * k + 3) % 64, dabgpu.subchannel((5 * k) % (865 - 4 * k), 8 * k, level=4))] if k else []


#: beyond 216 x 8 kbit/s EEP 4-A one sub-channel goes on as EEP 4-B (15 CUs per 32 kbit/s): 220, 224, 228 x 24 bytes
EEP_B_TOP = [55, 56, 57]


def eep_b_streams(n):
    return [(n, dabgpu.subchannel(864 - 15 * n, 32 * n, level=4, eep_type=1))]


def largest_frames():
    """-> {"length": streams of the longest frame, "data": streams of the frame with the most data bytes} that 864 CUs, 64
    streams and 6144 bytes allow.  Per CU a stream adds most as EEP 4-A at 8 kbit/s (its STC word and 24 bytes in 4 CUs) and
    as EEP 4-B (96 bytes in 15 CUs); every other profile adds less: the search is over the counts of 64 and 32 kbit/s EEP 4-B
    and 8 kbit/s EEP 4-A."""
    kinds = [(64, 1), (32, 1), (8, 0)]
    cu = [dabgpu.subchannel(0, br, level=4, eep_type=t).length for br, t in kinds]
    assert cu == [30, 15, 4]
    best_len, best_data = (0,), (0,)
    for a in range(65):
        for x in range(65 - a):
            y = min(64 - a - x, (864 - a * cu[0] - x * cu[1]) // cu[2])
            if y < 0:
                continue
            n, data = a + x + y, 192 * a + 96 * x + 24 * y
            length = 12 + 4 * n + 96 + data + 8
            if length > 6144:
                continue
            best_len = max(best_len, (length, a, x, y))
            best_data = max(best_data, (data, -n, a, x, y))

    def build(a, x, y):
        out, at = [], 0
        for k, (br, t) in enumerate([kinds[0]] * a + [kinds[1]] * x + [kinds[2]] * y):
            sc = dabgpu.subchannel(at, br, level=4, eep_type=t)
            out.append(((11 * k + 5) % 64, sc))
            at += sc.length
        return out[::2] + out[1::2]                               # (neither in id nor in address order)
    return {"length": build(*best_len[1:]), "data": build(*best_data[2:])}


LARGEST_LENGTH, LARGEST_DATA = 5884, 5520                        # bytes before the padding / data bytes: what the search finds


def test_eti_sweep_reaches_every_fold_shape(built):
    sweep = {fold_shape(dabgpu.eti_layout(sweep_streams(k))) for k in range(217)}
    assert len(sweep) == 217 and {c for c, _ in sweep} == set(range(1, 22))
    # every lead a chunk count can have: n_words = 24 + 6 k runs through every even number of its range
    for c in range(1, 22):
        assert {l for cc, l in sweep if cc == c} == {64 * c - n for n in range(24, 24 + 6 * 216 + 1, 6) if 64 * (c - 1) < n <= 64 * c}
    assert all(dabgpu.eti_layout(sweep_streams(k)).data_bytes == 24 * k for k in range(217))
    # every legal plan of ONE sub-channel -- every EEP profile at every bit rate that fits 864 CUs, every UEP row -- has a shape
    # of the sweep, or is one of the three EEP 4-B sizes beyond it
    top = {fold_shape(dabgpu.eti_layout(eep_b_streams(n))) for n in EEP_B_TOP}
    assert top == {(21, 0), (22, 40), (22, 16)} and not top & sweep      # 1344 = 21 x 64, 1368 and 1392 words
    legal = set()
    for level in (1, 2, 3, 4):
        for br in range(8, 1729, 8):
            sc = dabgpu.subchannel(0, br, level=level)
            if sc.length <= 864:
                legal.add(fold_shape(dabgpu.eti_layout([(1, sc)])))
        for br in range(32, 1825, 32):
            sc = dabgpu.subchannel(0, br, level=level, eep_type=1)
            if sc.length <= 864:
                legal.add(fold_shape(dabgpu.eti_layout([(1, sc)])))
    for index in range(64):
        legal.add(fold_shape(dabgpu.eti_layout([(1, dabgpu.uep_subchannel(index, 0))])))
    assert legal <= sweep | top and top <= legal
    with pytest.raises(dabgpu.DabGpuError):
        dabgpu.eti_layout([(1, dabgpu.subchannel(0, 32 * 58, level=4, eep_type=1))])      # 870 CUs


def test_largest_eti_frames(built):
    big = largest_frames()
    plan_l, plan_d = dabgpu.eti_layout(big["length"]), dabgpu.eti_layout(big["data"])
    assert (plan_l.length, plan_l.nst, plan_l.data_bytes) == (LARGEST_LENGTH, 62, LARGEST_DATA) and plan_d.nst == 31
    assert (plan_d.data_bytes, plan_d.length) == (LARGEST_DATA, 12 + 4 * plan_d.nst + 96 + LARGEST_DATA + 8)
    assert fold_shape(plan_l)[0] == fold_shape(plan_d)[0] == 22
    for streams in big.values():
        order = [sc.start_address for _i, sc in streams]
        assert order != sorted(order) and [i for i, _sc in streams] != sorted(i for i, _sc in streams)
        used = sum(sc.length for _i, sc in streams)
        assert used <= 864
        # ... and not one more of the smallest sub-channel fits: the CUs or the 64 streams have run out
        if len(streams) < 64:
            assert used + 4 > 864


def every_profile():
    """(CUs, bytes per CIF) of every sub-channel a Mode-I ensemble can hold: EEP 1..4-A at 8 n kbit/s, EEP 1..4-B at 32 n kbit/s,
    the 64 UEP rows -- sizes from dabgpu.subchannel / dabgpu.uep_subchannel, each accepted by dabgpu.eti_layout"""
    scs = [dabgpu.subchannel(0, br, level=lv) for lv in (1, 2, 3, 4) for br in range(8, 1729, 8)]
    scs += [dabgpu.subchannel(0, br, level=lv, eep_type=1) for lv in (1, 2, 3, 4) for br in range(32, 1825, 32)]
    scs += [dabgpu.uep_subchannel(index, 0) for index in range(64)]
    out = set()
    for sc in scs:
        if sc.length <= 864:
            assert dabgpu.eti_layout([(1, sc)]).data_bytes == 3 * sc.bitrate_kbps
            out.add((sc.length, 3 * sc.bitrate_kbps))
    return sorted(out)


def test_no_legal_ensemble_beats_the_largest_frames(built):
    """largest_frames() searches three profiles because every other adds less per CU; here that is checked, and the search is
    done again over EVERY profile: best[n][c] = the most a frame gains (4 bytes of STC and its data per stream, or the data
    alone) from n streams in c CUs."""
    profiles = every_profile()
    assert len(profiles) > 500 and (4, 24) in profiles and (15, 96) in profiles and (30, 192) in profiles
    # per CU: nothing adds more to the frame's length than 8 kbit/s EEP 4-A (28 bytes in 4 CUs), nothing more data than EEP 4-B
    assert max((b + 4) / cu for cu, b in profiles) == 7.0 and max(b / cu for cu, b in profiles) == 96 / 15
    assert {(cu, b) for cu, b in profiles if b / cu == 96 / 15} == {(15 * n, 96 * n) for n in range(1, 58)}
    for gain, want in ((lambda b: b + 4, LARGEST_LENGTH - 116), (lambda b: b, LARGEST_DATA)):
        item = {}
        for cu, b in profiles:                                       # (of two profiles of one size the larger gain)
            item[cu] = max(item.get(cu, 0), gain(b))
        best = np.full((65, 865), -1, np.int64)
        best[0, 0] = 0
        for n in range(1, 65):
            for cu, g in item.items():
                prev = best[n - 1, :865 - cu]
                np.maximum(best[n, cu:], np.where(prev >= 0, prev + g, -1), out=best[n, cu:])
        # the longest frame is 116 + 5768 = 5884 bytes: the 6144 of the frame never binds, the CUs run out first
        assert int(best.max()) == want and 116 + 4 * 64 + int(best.max()) <= 6144


def scrambled_small(n):
    """n sub-channels of 24 bytes, ids and start addresses scrambled, listed in neither order"""
    out = [((37 * i + 11) % 64, dabgpu.subchannel(4 * ((29 * i + 5) % n) + ((29 * i + 5) % n // 8) * 11, 8, level=4)) for i in range(n)]
    ids, starts = [i for i, _sc in out], [sc.start_address for _i, sc in out]
    assert len(set(ids)) == n == len(set(starts)) and ids != sorted(ids) and starts != sorted(starts)
    return out


def one_large(nst):
    """one sub-channel of 1920 bytes among nst - 1 of 24, the large one neither first nor last in the frame"""
    small = [(2 * k + 1, dabgpu.subchannel(600 + 8 * k if k else 0, 8, level=4)) for k in range(nst - 1)]
    return small[:1] + [(40, dabgpu.subchannel(100, 640, level=3))] + small[1:]


# ================================================================================================================ ETI: GPU
@pytest.fixture(scope="module")
def ectx(built):
    c = make_ctx(None, max_frames=160)
    yield c
    c.close()


def eti_round_trip(ctx, streams, n_streams, n_frames, seed, out_shift=0):
    rng = np.random.default_rng(seed)
    fib, ok, outs = make_case(rng, streams, n_streams, 4 * n_frames, [4990 + 7 * s + seed % 100 for s in range(n_streams)])
    eti, status, hist = run_eti(ctx, streams, fib, ok, outs, out_shift=out_shift)
    check_against_reference(streams, fib, ok, outs, eti, status, hist_out=hist)
    return eti, status


@pytest.mark.gpu
def test_gpu_eti_every_data_size_of_one_subchannel(ectx):
    """every (chunk_words, lead) of the data CRC: 0 .. 216 x 24 bytes as EEP 4-A, then the three EEP 4-B sizes beyond; one
    stream, one transmission frame each.  Nothing is thinned out."""
    for k in range(217):
        eti, status = eti_round_trip(ectx, sweep_streams(k), 1, 1, 1000 + k, out_shift=8 * (k % 2))
        assert int(status[0, 0]["length"]) == 12 + (4 if k else 0) + 96 + 24 * k + 8
    for n in EEP_B_TOP:
        eti_round_trip(ectx, eep_b_streams(n), 1, 1, 2000 + n)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["length", "data"])
def test_gpu_eti_largest_frames(ectx, which):
    streams = largest_frames()[which]
    eti, status = eti_round_trip(ectx, streams, 2, 1, 3000, out_shift=8)
    assert int(status[1, 3]["length"]) == dabgpu.eti_layout(streams).length


@pytest.mark.gpu
@pytest.mark.parametrize("nst", [63, 64])
def test_gpu_eti_63_and_64_small_subchannels(ectx, nst):
    eti_round_trip(ectx, scrambled_small(nst), 2, 2, 3100 + nst, out_shift=8)


@pytest.mark.gpu
@pytest.mark.parametrize("nst", [3, 4])
def test_gpu_eti_one_large_subchannel_on_either_lds_parity(ectx, nst):
    eti_round_trip(ectx, one_large(nst), 2, 2, 3200 + nst, out_shift=8)
    eti_round_trip(ectx, one_large(nst), 1, 1, 3300 + nst)


def first_fib(count):
    """a first FIB that begins with FIG 0/0 of this CIF count"""
    return synth.pack_fibs([synth.fig0_0(0xC181, count % 5000), bytes([0x3D]) + bytes(29)])[0]


def anchored_case(rng, fps, anchors, starts):
    """two `tiny` streams of 4 fps CIFs whose first FIBs are invalid -- CRC flag 0 at odd CIFs, a FIG 0/1 in front at even
    ones -- except at the CIFs of anchors[s].  The first of them says starts[s] + c; every later one says 1234 more, so which
    one the call took shows in every frame's count."""
    streams = CONFIGS["tiny"]()
    n_cif = 4 * fps
    fib, ok, outs = make_case(rng, streams, 2, n_cif, starts)
    for s in range(2):
        for c in range(n_cif):
            if c in anchors[s]:
                if c != min(anchors[s]):
                    fib[s, c, 0] = first_fib(starts[s] + c + 1234)
            elif c % 2:
                ok[s, c, 0] = 0
            else:
                fib[s, c, 0, 1] = 0x01
            assert (R.fig0_0_count(fib[s, c, 0], ok[s, c, 0]) is not None) == (c in anchors[s])
    return streams, fib, ok, outs


#: frames per stream, the anchors of stream 0 and of stream 1, d_cif_start
ANCHOR_CASES = {
    "255 | 256": (65, [255], [256], None),
    "257 | 256 and 3": (65, [257], [256, 3], None),
    "257 and 200 | 259 and 255": (65, [257, 200], [259, 255], None),       # a second-trip hit of a low thread, a first-trip hit of a high one
    "300 | 300 and 258": (80, [300], [300, 258], None),
    "511 and 260 | none": (129, [511, 260], [], None),
    "256 | 257 overridden": (65, [256], [257], [-1, 4321]),
}
LONG_STARTS = [4757, 4758]                                          # 4999 -> 0 between output frames 257 and 258 / 256 and 257


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ANCHOR_CASES))
def test_gpu_eti_anchor_beyond_256_cifs(ectx, name):
    fps, a0, a1, cif_start = ANCHOR_CASES[name]
    rng = np.random.default_rng(fps + len(a0) + 7 * len(a1))
    streams, fib, ok, outs = anchored_case(rng, fps, [a0, a1], LONG_STARTS)
    eti, status, hist = run_eti(ectx, streams, fib, ok, outs, cif_start=cif_start)
    ref_h = check_against_reference(streams, fib, ok, outs, eti, status, cif_start=cif_start, hist_out=hist)
    for s, anchors in enumerate([a0, a1]):
        if cif_start is not None and cif_start[s] >= 0:
            base = cif_start[s]
        else:
            base = LONG_STARTS[s] if anchors else 0
            assert bool((status[s]["flags"] & dabgpu.ETI_NO_ANCHOR).all()) == (not anchors)
            assert bool((status[s]["flags"] & dabgpu.ETI_NO_ANCHOR).any()) == (not anchors)
        assert list(status[s]["cif_count"].astype(int)) == [(base - 15 + t) % 5000 for t in range(4 * fps)]
        if base == LONG_STARTS[s]:
            wrap = 5000 - base + 15
            assert wrap > 256 and (status[s, wrap - 1]["cif_count"], status[s, wrap]["cif_count"]) == (4999, 0)
        mism = {int(t) - 15 for t in np.flatnonzero(status[s]["flags"] & dabgpu.ETI_COUNT_MISMATCH)}
        assert mism == {c for c in anchors if c < 4 * fps - 15 and (c != min(anchors) or base != LONG_STARTS[s])}
    # the call continued from its history by another 260 CIFs: stream 0 without an anchor (every thread's search comes back
    # empty and the count goes on from the record), stream 1 with one at CIF 261 - 256 = 5
    nxt = [int(h["next_count"]) for h in ref_h]
    streams, fib2, ok2, outs2 = anchored_case(rng, 65, [[], [5]], nxt)
    eti2, status2, hist2 = run_eti(ectx, streams, fib2, ok2, outs2, history=hist)
    check_against_reference(streams, fib2, ok2, outs2, eti2, status2, history=ref_h, hist_out=hist2)
    assert list(status2[0]["cif_count"].astype(int)) == [(nxt[0] - 15 + t) % 5000 for t in range(260)]
    assert (status2[0]["flags"] & dabgpu.ETI_NO_ANCHOR).all() and not (status2["flags"] & dabgpu.ETI_WARMUP).any()
    assert not (status2[1]["flags"] & dabgpu.ETI_NO_ANCHOR).any()


@pytest.mark.gpu
@pytest.mark.parametrize("fps", [65, 129])
def test_gpu_eti_no_anchor_in_a_long_call_with_a_history(ectx, fps):
    """no valid FIG 0/0 in either stream of a call of 260 / 516 CIFs, and the history record a call of 16 CIFs wrote handed in:
    the search of every thread, second and third trip included, finds nothing, the count goes on from the record's
    next_count (through 4999 -> 0 behind output frame 256), frames 0 .. 14 carry the record's FIC, and the call's own history
    out continues a third call the same way"""
    rng = np.random.default_rng(fps)
    starts = [LONG_STARTS[0] - 16, LONG_STARTS[1] - 16]
    streams, fib, ok, outs = anchored_case(rng, 4, [[2], [3]], starts)
    eti, status, hist = run_eti(ectx, streams, fib, ok, outs)
    ref_h = check_against_reference(streams, fib, ok, outs, eti, status, hist_out=hist)
    nxt = [int(h["next_count"]) for h in ref_h]
    assert nxt == LONG_STARTS and [int(h) for h in hist["valid"]] == [15, 15]
    for _ in range(2):
        streams, fib, ok, outs = anchored_case(rng, fps, [[], []], nxt)
        eti, status, hist2 = run_eti(ectx, streams, fib, ok, outs, history=hist)
        ref_h = check_against_reference(streams, fib, ok, outs, eti, status, history=ref_h, hist_out=hist2)
        for s in range(2):
            counts = [(nxt[s] - 15 + t) % 5000 for t in range(4 * fps)]
            assert list(status[s]["cif_count"].astype(int)) == counts
            assert (status[s]["flags"] & dabgpu.ETI_NO_ANCHOR).all() and not (status[s]["flags"] & (dabgpu.ETI_WARMUP | dabgpu.ETI_COUNT_MISMATCH)).any()
            assert int(hist2[s]["next_count"]) == (nxt[s] + 4 * fps) % 5000 and int(hist2[s]["valid"]) == 15
        if nxt == LONG_STARTS:                                         # the first long call: 4999 -> 0 behind output frame 256
            assert (int(status[0, 257]["cif_count"]), int(status[0, 258]["cif_count"])) == (4999, 0)
        nxt, hist = [int(h["next_count"]) for h in ref_h], hist2


DAMAGED_VALID = [-1, 0, 1, 14, 15, 16, 2 ** 31 - 1]
DAMAGED_COUNT = [-1, 4999, 5000, 2 ** 31 - 1]


def test_history_of_record_reads_what_the_header_says(built):
    fib = np.arange(15 * 96, dtype=np.uint32).astype(np.uint8).reshape(15, 96)
    ok = np.ones((15, 3), np.uint8)
    assert [len(R.history_of_record(fib, ok, 7, v)["fibs"]) for v in DAMAGED_VALID] == [0, 0, 1, 14, 15, 15, 15]
    assert [R.history_of_record(fib, ok, c, 1)["next_count"] % 5000 for c in DAMAGED_COUNT] == [2295, 4999, 0, 3647]
    h = R.history_of_record(fib, ok, 0, 2)
    assert np.concatenate([x.reshape(-1) for x in h["fibs"]]).tobytes() == fib[13:].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("fps", [1, 3, 4])
def test_gpu_eti_history_records_a_caller_hands_in_damaged(ectx, fps):
    """every valid x every next_count, one stream each, no anchor in the call: the record is read as include/dabgpu.h says.
    In calls of 4 and 12 CIFs the new record takes slots over from the old one; in a call of 16 it does not."""
    rng = np.random.default_rng(77 + fps)
    cases = [(v, c) for v in DAMAGED_VALID for c in DAMAGED_COUNT]
    n = len(cases)
    streams, n_cif = CONFIGS["tiny"](), 4 * fps
    fib, ok, outs = make_case(rng, streams, n, n_cif, [100] * n)
    fib[:, :, 0, 1] = 0x01                                           # no first FIB begins with FIG 0/0
    rec = np.zeros(n, dabgpu.ETI_HISTORY_DTYPE)
    rec["fib"] = rng.integers(0, 256, rec["fib"].shape, dtype=np.uint8)
    rec["crc_ok"] = rng.integers(0, 2, rec["crc_ok"].shape, dtype=np.uint8)
    for s in range(0, n, 3):                                         # some slots hold a FIG 0/0 of their own
        rec["fib"][s, :, :32] = [first_fib(40 * s + j) for j in range(15)]
        rec["crc_ok"][s, :, 0] = 1
    rec["valid"], rec["next_count"] = [v for v, _c in cases], [c for _v, c in cases]
    history = [R.history_of_record(rec[s]["fib"], rec[s]["crc_ok"], rec[s]["next_count"], rec[s]["valid"]) for s in range(n)]
    eti, status, hist = run_eti(ectx, streams, fib, ok, outs, history=rec)
    check_against_reference(streams, fib, ok, outs, eti, status, history=history, hist_out=hist)
    for s, (v, c) in enumerate(cases):
        held = min(max(v, 0), 15)
        base = (c & 0xFFFFFFFF) % 5000 if held else 0
        assert list(status[s]["cif_count"].astype(int)) == [(base - 15 + t) % 5000 for t in range(n_cif)]
        assert [bool(f & dabgpu.ETI_WARMUP) for f in status[s]["flags"]] == [t < 15 - held for t in range(n_cif)]
        assert int(hist[s]["valid"]) == min(held + n_cif, 15) and int(hist[s]["next_count"]) == (base + n_cif) % 5000
        assert not hist[s]["fib"][:15 - min(held + n_cif, 15)].any()    # (the slots that hold no CIF are zero, not the old record's bytes)


def split_calls(ctx, soft, streams, cut):
    """decode_frames_eti in one call and in calls of `cut` frames and the rest, the history handed on -> frames and status of
    both, on the host"""
    import torch
    one, st_one, _ = ctx.decode_frames_eti(soft, 1, streams)
    a, st_a, hist = ctx.decode_frames_eti(soft[:cut], 1, streams)
    b, st_b, _ = ctx.decode_frames_eti(soft[cut:], 1, streams, history=hist)
    status = lambda x: x.cpu().numpy().view(dabgpu.ETI_STATUS_DTYPE).reshape(-1)
    return one.cpu().numpy()[0], status(st_one), torch.cat([a, b], 1).cpu().numpy()[0], status(torch.cat([st_a, st_b], 1))


@pytest.mark.gpu
def test_gpu_decode_frames_eti_on_65_transmitted_frames(ectx):
    """65 frames of the service chain (test_eti.py's, transmitted on: its first 20 frames are that chain's), 260 CIFs: one call
    equals calls of 64 + 1 with the history handed on, byte for byte, and every frame behind the warm-up is the reference
    writer's frame of the TRANSMITTED FIBs and sub-channel bytes"""
    import torch
    from test_eti import DAB_SERVICES, SERVICES, ref_stream
    ens = synth.ServiceEnsemble(7, SERVICES, n_frames=65, dab_services=DAB_SERVICES, extras=False)
    soft, _, _ = ectx.ofdm_demod_frames(np.ascontiguousarray(ens.iq()[:, synth.NB_NULL:]), np.zeros(65, np.float32))
    scs = {3: dabgpu.subchannel(0, 64, level=3), 7: dabgpu.subchannel(48, 48, level=2),
           9: dabgpu.subchannel(200, 32, level=2, eep_type=1), 11: dabgpu.uep_subchannel(17, 100)}
    streams = [(9, scs[9]), (3, scs[3]), (11, scs[11]), (7, scs[7])]
    sent = {3: ens.msc_bytes[0], 7: ens.msc_bytes[1], 9: ens.msc_bytes[2], 11: ens.mp2_frames[0]}
    one, st_one, two, st_two = split_calls(ectx, torch.from_numpy(soft).cuda(), streams, 64)
    assert one.shape == (260, 6144) and (one == two).all() and st_one.tobytes() == st_two.tobytes()
    ref = [ref_stream(i, sc) for i, sc in streams]
    fibs = ens.fibs.reshape(260, 3, 32)
    assert list(st_one["cif_count"].astype(int)) == [(t - 15) % 5000 for t in range(260)]
    assert [int(f) for f in st_one["flags"]] == [dabgpu.ETI_WARMUP] * 15 + [0] * 245
    for t in range(15, 260):
        c = t - 15
        assert one[t].tobytes() == R.write_frame(ref, c, fibs[c].tobytes(), {i: sent[i][c] for i in sent}, 0xFF), t


@pytest.mark.gpu
def test_gpu_decode_frames_eti_on_65_frames_of_repeated_soft_bits(ectx, service_chain):
    """the service chain's 20 frames of soft bits repeated to 65, in one call and in calls of 64 + 1.  The FIC's own count
    starts again every 80 CIFs, and a call takes its count from its OWN first FIG 0/0 (include/dabgpu.h, "CIF count"): the
    first 64 frames' output is the same either way, and the last call's four frames are the one call's with the count the
    last call anchors on -- CIF 16 is its first -- and nothing else changed."""
    import torch
    from test_eti import ref_stream
    _ens, soft, streams, _sent = service_chain
    one, st_one, two, st_two = split_calls(ectx, torch.cat([soft] * 4)[:65].contiguous(), streams, 64)
    assert one.shape == (260, 6144) and (one[:256] == two[:256]).all() and st_one[:256].tobytes() == st_two[:256].tobytes()
    assert list(st_one["cif_count"].astype(int)) == [(t - 15) % 5000 for t in range(260)]
    assert [bool(f & dabgpu.ETI_WARMUP) for f in st_one["flags"]] == [t < 15 for t in range(260)] and (st_one["fib_ok"][15:] == 7).all()
    # from CIF 80 on a frame's own FIG 0/0 says the count of 80, 160, 240 CIFs before
    own = [R.fig0_0_count(dabgpu.eti_parse(one[t])["fic"][:32], 1) for t in range(15, 260)]
    assert own == [c % 80 for c in range(245)]
    assert [bool(f & dabgpu.ETI_COUNT_MISMATCH) for f in st_one["flags"][15:]] == [c >= 80 for c in range(245)]
    ref = [ref_stream(i, sc) for i, sc in streams]
    for t in range(256, 260):
        info = dabgpu.eti_parse(one[t])
        count = 16 - 15 + (t - 256)                                  # = the count the FIC of CIF t - 15 carries: 241 % 80 = 1
        want = R.write_frame(ref, count, info["fic"].tobytes(), {x["scid"]: x["data"].tobytes() for x in info["streams"]}, info["err"])
        assert two[t].tobytes() == want, t
        assert (int(st_two[t]["cif_count"]), int(st_two[t]["flags"]), int(st_two[t]["fib_ok"])) == (count, 0, 7)


# ============================================================================================================ the census
#: Every loop of the ETI, align / follow, PAD and MOT kernels whose trip count a CALL ARGUMENT sets (loops over what the data
#: says -- access units, PAD lengths, copy orders -- belong to test_pad_device_edges.py's census of copy orders).
#: (file, the loop as written, argument, {trips: (smallest argument, the test that reaches that trip count -- at the
#: argument in brackets where it is not the smallest -- or None where no argument can give it)})
_B, _F, _E, _P = "test_beyond_one_wave.py::", "test_dabplus_follow.py::", "test_eti.py::", "test_pad_device_edges.py::"
_SWEEP = _B + "test_gpu_eti_every_data_size_of_one_subchannel"
CENSUS = [
    ("eti_kernels.hip", "for (int c = tid; c < n_cif; c += ETI_WG)", "n_cif = 4 frames_per_stream, per thread",
     {"0": ("any: threads >= n_cif", _E + "test_odd_shapes"), "1": ("frames_per_stream = 1", _E + "test_odd_shapes"),
      "2": ("frames_per_stream = 65 (threads 0..3)", _B + "test_gpu_eti_anchor_beyond_256_cifs"),
      "ragged": ("65: 4 of 256 threads; a third trip at 129: 4 threads", _B + "test_gpu_eti_no_anchor_in_a_long_call_with_a_history")}),
    ("eti_kernels.hip", "for (int k = 0; k < a.nst; k++)", "nst",
     {"0": ("nst = 0", _E + "test_odd_shapes"), "1": ("nst = 1", _E + "test_odd_shapes"),
      "2": ("nst = 2 [3]", _B + "test_gpu_eti_one_large_subchannel_on_either_lds_parity"),
      "ragged": ("none: one trip per stream [`tid < a.nst`, `lane < a.nst` at 63, 64]", _B + "test_gpu_eti_63_and_64_small_subchannels")}),
    ("eti_kernels.hip", "for (int w = tid; w < n; w += ETI_WG) s_map[first + w] = uint8_t(k);", "bytes[k] / 8, per thread",
     {"0": ("any: threads >= 3 at 24 bytes", _SWEEP), "1": ("24 bytes", _SWEEP), "2": ("2056 bytes: 2064 = 86 x 24", _SWEEP),
      "ragged": ("every size but 2048 n", _SWEEP)}),
    ("eti_kernels.hip", "for (int w0 = lane; w0 < n_w8; w0 += 4 * 64)", "data_bytes / 8, per lane",
     {"0": ("data_bytes = 0", _SWEEP), "1": ("24", _SWEEP), "2": ("2064 (n_w8 = 258)", _SWEEP),
      "ragged": ("every size but 2048 n; the four loads of a trip: every n_w8 mod 256", _SWEEP)}),
    ("eti_kernels.hip", "for (int j = 0; j < a.chunk_words; j++)", "chunk_words = ceil((24 + data_bytes / 4) / 64)",
     {"0": ("never: the FIC alone is 24 words", None), "1": ("data_bytes = 0 .. 144", _SWEEP), "2": ("168", _SWEEP),
      "ragged": ("lead = 64 chunk_words - n_words: every value", _SWEEP)}),
    ("dabplus_kernels.hip", "for (int i0 = 0; i0 < T; i0 += 64)", "T = held + n_cifs",
     {"0": ("n_cifs = 0, held = 0", _B + "test_gpu_follow_table_growth_and_no_cifs"), "1": ("1", _F + "test_gpu_alignment_and_chunking"),
      "2": ("65", _B + "test_gpu_follow_block_boundaries"), "ragged": ("T mod 64 != 0: 65, 69, 129, 133", _B + "test_gpu_follow_block_boundaries")}),
    ("dabplus_kernels.hip", "for (int j = 0; j < kept; j++)", "kept = T - first_kept (0..4)",
     {"0": ("T = phase mod 5", _B + "test_gpu_follow_block_boundaries"), "1": ("one more", _B + "test_gpu_follow_block_boundaries"),
      "2": ("two more", _B + "test_gpu_follow_block_boundaries"), "ragged": ("none", None)}),
    ("dabplus_kernels.hip", "for (int i = kept * lf / 8 + lane; i < 4 * lf / 8; i += 64)", "(4 - kept) 3 s words, per lane",
     {"0": ("kept = 4", _B + "test_gpu_follow_block_boundaries"), "1": ("s = 1", _B + "test_gpu_follow_block_boundaries"),
      "2": ("s = 6, kept = 0 [8]", _B + "test_gpu_follow_block_boundaries"), "ragged": ("s = 8: 96 words [12 trips at s = 64]", _B + "test_gpu_follow_large_s")}),
    ("dabplus_kernels.hip", "for (int i = lane; i < n / 16; i += 64)", "n = 24 s, s even, everything on 16 bytes",
     {"0": ("never", None), "1": ("s = 2", _B + "test_gpu_follow_table_growth_and_no_cifs"), "2": ("s = 44 [48]", _B + "test_gpu_follow_large_s"),
      "ragged": ("s = 44 [48: 72 words]", _B + "test_gpu_follow_large_s")}),
    ("dabplus_kernels.hip", "for (int i = lane; i < n / 8; i += 64)", "n = 24 s, on 8 bytes",
     {"0": ("never", None), "1": ("s = 1", _F + "test_gpu_alignment_and_chunking"), "2": ("s = 22 [25]", _B + "test_gpu_follow_large_s"),
      "ragged": ("s = 22 [25: 75 words; 63: 189]", _B + "test_gpu_follow_large_s")}),
    ("dabplus_kernels.hip", "for (int i = lane; i < n; i += 64) dst[i] = src[i];", "n = 24 s, bytes",
     {"0": ("never", None), "1": ("s = 1", _F + "test_gpu_alignment_and_chunking"), "2": ("s = 3", _B + "test_gpu_follow_ragged_s_in_one_call"),
      "ragged": ("s = 1: 24 bytes", _F + "test_gpu_alignment_and_chunking")}),
    ("dabplus_kernels.hip", "if (k >= pl.n_superframes) return;", "the grid: n_entries x max_sf, max_sf = (n_cifs + 4) / 5",
     {"0": ("n_cifs = 0: no launch", _B + "test_gpu_follow_table_growth_and_no_cifs"), "1": ("1 x 1", _F + "test_gpu_alignment_and_chunking"),
      "2": ("n_cifs = 6 [7]", _F + "test_gpu_alignment_and_chunking"),
      "ragged": ("whole rows idle: an all-erasure entry among 200 x 14", _B + "test_gpu_follow_table_growth_and_no_cifs")}),
    ("dabplus_kernels.hip", "for (int i = tid; i < 110 * s; i += 64) dst[i] = sf[i];", "s (the super-frame body's loops over 110 s, 120 s, s columns)",
     {"0": ("never", None), "1": ("never: 110 bytes", None), "2": ("s = 1", "test_dabplus_superframes.py::test_gpu_every_bitrate"),
      "ragged": ("every s but 32 and 64 [through the follow call: 25 .. 63]", _B + "test_gpu_follow_large_s")}),
    ("pad_kernels.hip", "for (int k = 0; k < n_sf; k++)", "n_superframes of the follow record, capped by max_superframes",
     {"0": ("0 (and -1)", _P + "test_gpu_n_superframes_as_the_label_call_reads_it"), "1": ("1", _P + "test_gpu_every_cut_in_two_launches_labels"),
      "2": ("2", _P + "test_gpu_every_cut_in_two_launches_labels"), "ragged": ("none", None)}),
    ("mot_kernels.hip", "for (int k = 0; k < n_sf; k++)", "n_superframes of the follow record, capped by max_superframes",
     {"0": ("0 (and -1)", _P + "test_gpu_n_superframes_as_the_slide_call_reads_it"), "1": ("1", _P + "test_gpu_every_cut_in_two_launches_slides"),
      "2": ("2", _P + "test_gpu_every_cut_in_two_launches_slides"), "ragged": ("none", None)}),
]
#: loops of those files that no call argument reaches: constant trip counts, or counts the DATA sets
NOT_ARGUMENT_LOOPS = {
    "eti_kernels.hip": ["for (int i = bits - 1; i >= 0; i--)", "for (int i = tid; i < ETI_FIC_DELAY * ETI_FIC_WORDS; i += ETI_WG)",
                        "for (int i = 0; i < 8; i++)", "for (int j = 0; j < ETI_FRAME_BYTES / 16 / 64; j++)", "for (int u = 0; u < 4; u++)",
                        "for (int d = 32; d >= 1; d >>= 1)"],
    "pad_kernels.hip": ["for (int a = 0; a < n_aus; a++)", "for (int i = 3 + lane; i < need; i += 64)", "for (int i = 0; i < n_entries; i++)"],
    "mot_kernels.hip": ["for (int a = 0; a < n_aus; a++)", "for (int i = 3 + lane; i < need; i += 64)", "for (int i = 0; i < n_orders; i++)",
                        "for (int j = lane; j < o.len; j += 64)", "for (int i = 0; i < n_entries; i++)"],
}


def test_census_of_argument_dependent_loops(built):
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("eti_kernels.hip", "dabplus_kernels.hip", "pad_kernels.hip", "mot_kernels.hip")}
    readme = open(os.path.join(TESTS, "README.md")).read()
    for f, loop, _arg, trips in CENSUS:
        assert loop in src[f], (f, loop)
        assert sorted(trips) == ["0", "1", "2", "ragged"]
        for what, t in trips.values():
            # a trip count has its test, unless no argument can give it
            assert (t is None) == (what.startswith("never") or what == "none"), (loop, what)
            if t is not None:
                mod, name = t.split("::")
                assert re.search(r"^def %s\(" % re.escape(name), open(os.path.join(TESTS, mod)).read(), re.M), t
                assert "`%s`" % t in readme, "tests/README.md does not name " + t
        assert "`%s`" % loop in readme, "tests/README.md does not list " + loop
    # no loop of the ETI, PAD and MOT kernels is left out: each is in the census or named as not argument-dependent
    for f in ("eti_kernels.hip", "pad_kernels.hip", "mot_kernels.hip"):
        listed = [l for ff, l, *_ in CENSUS if ff == f] + NOT_ARGUMENT_LOOPS[f]
        for m in re.finditer(r"for \([^\n]*?\)(?= |\n|$)", src[f]):
            head = m.group(0)
            assert any(l.startswith(head) or head.startswith(l) for l in listed), (f, head)
    # the align and follow kernels' part of dabplus_kernels.hip
    tail = src["dabplus_kernels.hip"][src["dabplus_kernels.hip"].index("following a sub-channel"):src["dabplus_kernels.hip"].index("launch_dabplus_superframes(")]
    listed = [l for ff, l, *_ in CENSUS if ff == "dabplus_kernels.hip"] + ["for (int q = 0; q < 5; q++)", "for (int q = 4; q >= 0; q--)",
                                                                          "for (int j = 0; j < 5; j++)"]
    for m in re.finditer(r"for \([^\n]*?\)(?= |\n|$)", tail):
        assert any(l.startswith(m.group(0)) for l in listed), m.group(0)
    # what the census says of the new inputs holds of them
    assert set(BOUNDARY_CIFS) == {59, 60, 63, 64, 65, 69, 124, 128, 129, 133} and set(BIG_S) == {25, 32, 37, 38, 47, 48, 63, 64}
    kept = {(sp["s"], decisions(sp)[5]) for n_cifs in BOUNDARY_CIFS for sp in boundary_specs(n_cifs)}
    assert kept == {(s, k) for s in (1, 8) for k in range(5)}         # every `kept` at both s: the carry's copy and zero-fill loops
    assert any(sp["s"] == 3 and sp["shift"] % 8 for sp in ragged_specs()) and any(sp["s"] == 2 and sp.get("stride", 48) % 16 == 0 for sp in growth_specs())
    assert any(sp["s"] == 25 and sp["stride"] == 600 and sp["shift"] == 0 for sp in big_s_specs(25)[0])
    assert RAGGED_S == [1, 64, 3, 48, 24, 25] and {sp["s"] for sp in growth_specs()} == {1, 2, 3}
    assert sum(sp["phase"] == -1 for sp in growth_specs()) >= GROWTH_ENTRIES // 3
    assert all(v[0] > 64 for v in ANCHOR_CASES.values()) and {v[0] for v in ANCHOR_CASES.values()} == {65, 80, 129}
    assert dabgpu.eti_layout(sweep_streams(86)).data_bytes == 2064 and fold_shape(dabgpu.eti_layout(sweep_streams(7)))[0] == 2
