"""The channel decoder (rows A8-A12 and f-2 of tests/README.md: depuncturing, the K = 7 rate-1/4 soft Viterbi, energy
dispersal, FIB CRC, the time de-interleaver, EEP-A / EEP-B / UEP) against tests/decoder_reference.py, an exact
from-definition reference with int64 path metrics that knows nothing of the oracle's or the kernels' start penalty,
renormalisation or tie rule.

`-m "not gpu"`: the reference earns its authority (exhaustive search, the numpy transmitter's round trips, equality
of its tables with the oracle's and the library's), the oracle is held to it on every input the GPU tests use, and
the input families are shown to be what they claim: the headroom family reaches a path-metric excursion of 9 906 (a
clean +-127 codeword of a random message), which max_excursion() shows to be the largest any input can reach, and the
signal-plus-noise families have a unique optimum on at least 90 % of their codewords.  The figures are printed (`-s` shows them).

`-m gpu`: every path of the decoder -- wave kernel, lane kernel with its prep kernel, the fused forward pass, the
grouped launch -- on the same inputs.  Every case asserts, in this order, so that a failure names its kind:
  1. metric_of(GPU bytes) == best: the output is A maximum-likelihood sequence (a failure is a decoding bug whatever
     the tie rule);
  2. GPU bytes == bits(documented tie rule): bit-exact (a failure with 1 passing is a tie-rule difference);
  3. FIC: the CRC flags equal the reference's.
No case is skipped and no codeword is left out of 1 and 2."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import decoder_reference as R
from conftest import golden_path, make_ctx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEPS_H = 606                                           # headroom and lure inputs: 600 information bits, unpunctured
CLEAN_EXCURSION = 9906                                   # a clean +-127 codeword of a random message (the issue's bar)
HEADER_BOUND = 12240                                     # viterbi_lane_kernels.hip: +-24 480 doubled


def max_excursion(period=12):
    """The largest excursion ANY input within +-127 can reach, from the code alone.  After `period` steps the best metric
    has grown by at most 4 * 127 a step.  At the reference step the state-0 metric lags the best metric by at most
    2 * 127 * D: if q is the best path and p any path into state 0, corr(q) - corr(p) = sum over the positions where they
    differ of at most 2 * 127 each, and by linearity the smallest number of such positions is the smallest weight of a
    path from the zero state into state(q) -- D is its largest value over the 64 states, found here by the reference
    on an all-zero codeword (D = 15).  A clean codeword whose state at a multiple of the period is one of those states
    attains it, so the bound is exact: 12 * 508 + 15 * 254 = 9 906, which is what a clean codeword of a random message
    reaches.  No input exceeds it; the seeded search of golden/make_decoder_headroom.py agrees (it climbs to 9 906 and
    stays).  The lane kernel's header bounds the same quantity by 12 240."""
    d = R.viterbi(np.full((1, 4 * 66), -127, np.int64))
    m = np.zeros((1, 64), np.int64)
    m[:] = R.NEG_INF
    m[:, 0] = 0
    for t in range(60):
        bm = np.full((1, 4), -127, np.int64) @ R._SIGNS
        m = np.maximum(m[:, R._PRED0] + bm[:, 0::2], m[:, R._PRED1] + bm[:, 1::2])
    assert d.best[0] == 4 * 127 * 66 and m[0, 0] == 4 * 127 * 60
    weight = (m[0, 0] - m[0]) // 254                     # smallest weight of a path from state 0 into each state
    return period * 4 * 127 + 254 * int(weight.max())


MAX_EXCURSION = max_excursion()


def _report(line):
    print("\n[decoder_reference] " + line)


# ================================================================================================ input families
def _clean(msgs, amp=127, **kw):
    return (R.conv_encode(msgs, **kw).astype(np.int64) * 2 - 1) * amp


def _signal_noise(rng, code_pm1, snr_db, amp):
    """+-amp + Gaussian noise of amp / 10^(dB / 20) per soft bit, rounded and clipped to int8's +-127."""
    sigma = amp / 10.0 ** (snr_db / 20.0)
    return np.clip(np.rint(code_pm1 * amp + rng.normal(0.0, sigma, code_pm1.shape)), -127, 127).astype(np.int64)


LONG_LENGTHS = (774, 3078, 27654)                        # the FIC, EEP 3-A 128 kbit/s, EEP 3-A filling the CIF
LONG_KINDS = ("pi1", "pi24", "real")
LONG_LANES = {774: 64, 3078: 64, 27654: 32}              # (the longest at half a group: the reference's run time)
LANE_KINDS = ("4dB", "8dB", "12dB", "20dB", "uniform", "grid", "4dB", "8dB", "12dB", "20dB", "zeros", "clean",
              "uniform", "grid", "4dB", "8dB")           # every lane of a group a different input
AMPLITUDE = {"pi1": 127, "pi24": 60, "real": 60}


def _long_mask(nsteps, kind):
    if kind == "real":
        return {774: R.fic_profile(), 3078: R.eep_profile(0, 3, 128), 27654: R.eep_profile(0, 3, 1152)}[nsteps].mask
    return R.plain_mask(nsteps, 1 if kind == "pi1" else 24)


@functools.lru_cache(maxsize=None)
def long_case(nsteps, kind):
    """-> mask, punctured soft bits int8 [lanes][kept], the lanes' kinds."""
    mask = _long_mask(nsteps, kind)
    sent = np.flatnonzero(mask)
    rng = np.random.default_rng([nsteps, LONG_KINDS.index(kind), 0xDEC])
    lanes = LONG_LANES[nsteps]
    kinds = [LANE_KINDS[i % len(LANE_KINDS)] for i in range(lanes)]
    msgs = rng.integers(0, 2, (lanes, nsteps - 6), dtype=np.uint8)
    code = (R.conv_encode(msgs).astype(np.int64) * 2 - 1)[:, sent]
    out = np.zeros((lanes, sent.size), np.int64)
    for i, k in enumerate(kinds):
        if k.endswith("dB"):
            out[i] = _signal_noise(rng, code[i], float(k[:-2]), AMPLITUDE[kind])
        elif k == "uniform":
            out[i] = rng.integers(-127, 128, sent.size)
        elif k == "grid":
            out[i] = rng.integers(-8, 8, sent.size) * 16 + 8                     # 16 levels: many exact ties
        elif k == "clean":
            out[i] = code[i] * 127
    return mask, out.astype(np.int8), kinds


@functools.lru_cache(maxsize=None)
def long_ref(nsteps, kind):
    mask, punct, _ = long_case(nsteps, kind)
    mother = R.depuncture(punct, mask)
    return mother, R.viterbi(mother)


def _burst(x, t, n):
    x[4 * t:4 * (t + n)] *= -1


@functools.lru_cache(maxsize=None)
def headroom_pool():
    """-> soft int8 [N][4 * 606] (N >= 257), family name per input.  Saturated (+-127) throughout."""
    rng = np.random.default_rng(0x4EAD)
    K = NSTEPS_H - 6
    rows, fam = [], []

    def add(x, name):
        rows.append(np.asarray(x, np.int64)); fam.append(name)

    alt = np.arange(K) % 2
    for m in (np.zeros(K), np.ones(K), alt, 1 - alt, (np.arange(K) // 2) % 2, (np.arange(K) // 6) % 2):
        add(_clean(m.astype(np.uint8))[0], "clean, patterned message")
    for _ in range(6):
        add(_clean(rng.integers(0, 2, K, dtype=np.uint8))[0], "clean, random message")
    for n in range(1, 13):                               # inverted bursts of 1 .. 12 steps at every phase of the period
        for phase in range(12):
            x = _clean(rng.integers(0, 2, K, dtype=np.uint8))[0]
            _burst(x, 12 * int(rng.integers(4, 40)) + phase, n)
            add(x, "inverted burst")
        x = _clean(rng.integers(0, 2, K, dtype=np.uint8))[0]
        _burst(x, K - n, n)                              # ... and just before the tail
        add(x, "inverted burst before the tail")
        x = _clean(rng.integers(0, 2, K, dtype=np.uint8))[0]
        _burst(x, NSTEPS_H - n, n)                       # ... and in it
        add(x, "inverted burst before the tail")
    for n in (6, 11, 12, 13, 24, 48, 96, 200):           # erasures, then saturated signal
        for t in (0, 12 * 10 + n % 12):
            for m in (rng.integers(0, 2, K, dtype=np.uint8), np.ones(K, np.uint8)):
                x = _clean(m)[0]
                x[4 * t:4 * (t + n)] = 0
                add(x, "erasures, then saturated signal")
    g = np.load(golden_path("decoder_headroom.npz"))
    for x in g["soft"]:
        add(x, "searched (decoder_headroom.npz)")
    while len(rows) < 257:                               # two bursts, patterned stretches in random messages
        m = rng.integers(0, 2, K, dtype=np.uint8)
        a = int(rng.integers(0, K - 60))
        m[a:a + int(rng.integers(6, 60))] = int(rng.integers(0, 2))
        x = _clean(m)[0]
        for _ in range(2):
            n = int(rng.integers(1, 13))
            _burst(x, int(rng.integers(0, NSTEPS_H - n)), n)
        add(x, "two bursts, patterned stretch")
    return np.stack(rows).astype(np.int8), fam


@functools.lru_cache(maxsize=None)
def headroom_ref():
    soft, _ = headroom_pool()
    return soft.astype(np.int64), R.viterbi(soft)


LURE_STATES = (63, 21, 42, 1, 32)


@functools.lru_cache(maxsize=None)
def lure_pool():
    """A transmitter that breaks the rule, at +-127: the whole input is the codeword of an encoder that STARTED in
    state s != 0 (so the first six steps run along the path that leaves s, and the rest is explained better by that
    path than by any path from state 0), or that ENDS in state s != 0 (six tail bits other than zeros).  What is
    right is decided by the reference's known start and end states."""
    rng = np.random.default_rng(0x105E)
    K = NSTEPS_H - 6
    rows, fam = [], []
    for s in LURE_STATES:
        for m in (rng.integers(0, 2, K, dtype=np.uint8), np.zeros(K, np.uint8), np.ones(K, np.uint8)):
            rows.append(_clean(m, start_state=s)[0]); fam.append("start state %d" % s)
            tail = np.array([(s >> (5 - k)) & 1 for k in range(6)], np.uint8)     # the last tail bit is state bit 5
            rows.append(_clean(m, tail=tail)[0]); fam.append("end state %d" % s)
            x = _clean(m, start_state=s, tail=tail)[0]
            x[24:] = np.where(rng.random(x.size - 24) < 0.05, -x[24:], x[24:])    # both, with a few bits inverted
            rows.append(x); fam.append("both %d" % s)
    return np.stack(rows).astype(np.int8), fam


@functools.lru_cache(maxsize=None)
def lure_ref():
    soft, _ = lure_pool()
    return soft.astype(np.int64), R.viterbi(soft)


CRC_VARIANTS = ("valid", "data bit", "crc bit", "crc 0000", "crc ffff")


@functools.lru_cache(maxsize=None)
def fic_case():
    """-> soft int8 [9][9216], the FIBs sent in frames 0 .. 2 [3][12][32], the CRC flags they must get [3][12]."""
    rng = np.random.default_rng(0xF1C)
    p = R.fic_profile()
    sent = np.flatnonzero(p.mask)
    fibs = np.zeros((5, 12, 32), np.uint8)
    flags = np.ones((5, 12), np.uint8)
    for f in range(5):
        for k in range(12):
            fib = R.fib_with_crc(rng.integers(0, 256, 30, dtype=np.uint8))
            v = CRC_VARIANTS[(f + k) % 5] if f < 3 else "valid"
            if v == "data bit":
                fib[int(rng.integers(0, 30))] ^= 1 << int(rng.integers(0, 8))
            elif v == "crc bit":
                fib[30 + int(rng.integers(0, 2))] ^= 1 << int(rng.integers(0, 8))
            elif v == "crc 0000":
                fib[30:] = 0
            elif v == "crc ffff":
                fib[30:] = 0xFF
            fibs[f, k] = fib
            flags[f, k] = R.fib_crc_ok(fib)
    assert flags[:3].sum() == 7 and flags[3:].all()      # (only the untouched FIBs pass: no variant hit its CRC by chance)
    bits = np.unpackbits(fibs.reshape(20, 96), axis=1) ^ R.prbs(768)[None, :]
    code = (R.conv_encode(bits).astype(np.int64) * 2 - 1)[:, sent].reshape(5, 9216)
    soft = np.zeros((9, 9216), np.int64)
    soft[:3] = code[:3] * 127                            # as sent: the decoder returns them as they are
    soft[3] = _signal_noise(rng, code[3], 4.0, 60)
    soft[4] = _signal_noise(rng, code[4], 8.0, 60)
    soft[5] = rng.integers(-127, 128, 9216)
    soft[6] = rng.integers(-8, 8, 9216) * 16 + 8
    soft[8] = rng.choice([-127, 127], 9216)              # (7: all erased)
    return soft.astype(np.int8), fibs[:3], flags[:3]


@functools.lru_cache(maxsize=None)
def fic_ref():
    return R.fic_reference(fic_case()[0])


# ---- MSC: three sub-channels, two streams of 49 frames, cut into calls of 1, 15, 16 and 17 frames -------------------
MSC_TYPES = ("eep_a", "eep_b", "uep")
MSC_FRAMES = 49
MSC_CUTS = (1, 15, 16, 17)
MSC_STARTS = {0: (0, 101, 829), 1: (101, 849, 0), 2: (840, 0, 101)}      # layout -> start CU of (EEP-A, EEP-B, UEP)


def msc_profile(kind):
    return {"eep_a": R.eep_profile(0, 3, 32), "eep_b": R.eep_profile(1, 4, 32), "uep": R.uep_profile(4)}[kind]


@functools.lru_cache(maxsize=None)
def msc_case(kind):
    """-> the sub-channel's soft bits int8 [2 streams][196 CIFs][size * 64], the logical frames sent [2][181][bytes].
    Stream 0 is saturated and clean (its de-interleaved codewords are headroom inputs), stream 1 signal at amplitude
    60 plus noise at 6 dB.  The UEP profile's padding bits carry noise: a decoder must not read them."""
    p = msc_profile(kind)
    rng = np.random.default_rng([MSC_TYPES.index(kind), 0x35C])
    T = 4 * MSC_FRAMES
    nbits = p.size_cu * 64
    sent = np.flatnonzero(p.mask)
    data = rng.integers(0, 256, (2, T - 15, p.nbytes), dtype=np.uint8)
    data[0, 3] = 0xFF
    data[0, 4] = 0
    soft = np.zeros((2, T, nbits), np.int64)
    for s in range(2):
        bits = np.unpackbits(data[s], axis=1) ^ R.prbs(8 * p.nbytes)[None, :]
        code = np.zeros((T - 15, nbits), np.int64)
        code[:, :p.kept] = (R.conv_encode(bits).astype(np.int64) * 2 - 1)[:, sent]
        tx = R.time_interleave(code)                     # [T][nbits]; 0 where no logical frame of these reaches
        soft[s] = tx * 127 if s == 0 else np.where(tx != 0, _signal_noise(rng, tx, 6.0, 60), 0)
        if p.padding:
            soft[s][:, p.kept:] = rng.integers(-127, 128, (T, nbits - p.kept))
    return soft.astype(np.int8), data


@functools.lru_cache(maxsize=None)
def msc_ref(kind):
    soft, _ = msc_case(kind)
    return [R.msc_reference(soft[s], None, msc_profile(kind)) for s in range(2)]


@functools.lru_cache(maxsize=None)
def msc_frames(layout):
    """Whole frames int8 [2 * 49][230400] (stream-major): noise everywhere, the three sub-channels at the layout's
    start addresses (0, an odd capacity unit, the last that fits)."""
    rng = np.random.default_rng(0xF4A + layout)
    soft = rng.integers(-127, 128, (2, MSC_FRAMES, 230400), dtype=np.int8)
    cifs = soft[:, :, R.NB_FIC_BITS:].reshape(2, 4 * MSC_FRAMES, R.NB_CIF_BITS)      # (a copy: the slice is not contiguous)
    for kind, start in zip(MSC_TYPES, MSC_STARTS[layout]):
        sub, _ = msc_case(kind)
        assert start + msc_profile(kind).size_cu <= 864
        cifs[:, :, 64 * start:64 * start + sub.shape[2]] = sub
    soft[:, :, R.NB_FIC_BITS:] = cifs.reshape(2, MSC_FRAMES, 4 * R.NB_CIF_BITS)
    return soft.reshape(2 * MSC_FRAMES, 230400)


@functools.lru_cache(maxsize=None)
def msc_fic_ref(layout):
    return R.fic_reference(msc_frames(layout))


# ================================================================================================ CPU: the reference
def test_reference_imports_neither_the_oracle_nor_the_library():
    code = ("import sys; sys.path[:0] = [%r, %r]; import decoder_reference as R; R.uep_profile(0); "
            "bad = [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.') or m in ('dabgpu', 'ctypes', 'torch')"
            " and getattr(sys.modules.get('dabgpu'), '_LIB', None) is not None]; "
            "assert 'oracle' not in sys.modules and 'oracle.oracle' not in sys.modules, sys.modules.keys(); "
            "import dabgpu; assert dabgpu._LIB is None; print('ok')"
            % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
    src = open(os.path.join(ROOT, "tests", "decoder_reference.py")).read()
    imports = [l.strip() for l in src.splitlines() if l.strip().startswith(("import ", "from "))]
    assert sorted(imports) == ["from dabgpu.synth import _UEP_TABLE", "import binascii", "import numpy as np"], imports


def test_reference_is_maximum_likelihood_by_exhaustive_search():
    """16 information bits: `best` is the largest correlation any of the 65 536 codewords reaches, `unique` says
    whether exactly one reaches it, both tie rules reach it -- on noise, half-erased noise and small integers."""
    k = 16
    msgs = ((np.arange(1 << k)[:, None] >> np.arange(k - 1, -1, -1)) & 1).astype(np.uint8)
    code = R.conv_encode(msgs).astype(np.int64) * 2 - 1                         # [65536][88]
    rng = np.random.default_rng(16)
    n = 60
    soft = rng.integers(-127, 128, (n, code.shape[1]))
    soft[1::3][rng.random(soft[1::3].shape) < 0.5] = 0
    soft[2::3] = rng.integers(-2, 3, soft[2::3].shape)
    corr = soft @ code.T
    d = R.viterbi(soft)
    assert (d.best == corr.max(axis=1)).all()
    assert (d.unique == ((corr == corr.max(axis=1)[:, None]).sum(axis=1) == 1)).all()
    assert 0.2 < d.unique.mean() < 0.9                                          # (both kinds of case are present)
    for rule in (R.DOCUMENTED, R.OPPOSITE):
        idx = (d.bits(rule).astype(np.int64) << np.arange(k - 1, -1, -1)).sum(axis=1)
        assert (corr[np.arange(n), idx] == d.best).all(), rule
        assert (R.metric_of(d.bytes(rule), soft) == d.best).all()
    same = (d.bits(R.DOCUMENTED) == d.bits(R.OPPOSITE)).all(axis=1)
    assert (same == d.unique).all()                                             # the rules part exactly where a tie is


def test_reference_tables_against_the_standards_known_answers():
    assert R.prbs(16).tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0]          # clause 10
    assert (R.prbs(1022)[:511] == R.prbs(1022)[511:]).all()
    assert R.TDI_DELAY.tolist() == [0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15]   # clause 12, table
    imp = R.conv_encode(np.array([[1] + [0] * 10], np.uint8)).reshape(-1, 4)[:7]
    for p, g in enumerate((0o133, 0o171, 0o145, 0o133)):
        assert int("".join(map(str, imp[:, p])), 2) == g
    assert R.fib_crc_ok(R.fib_with_crc(np.arange(30))) == 1
    for i in range(64):
        R.uep_profile(i)                                                         # both identities, every row
    for opt, brs in ((0, range(8, 393, 8)), (1, range(32, 385, 32))):
        for lvl in (1, 2, 3, 4):
            for br in brs:
                R.eep_profile(opt, lvl, br)                                      # asserts steps and capacity units


def _mask_dump(tmp_path):
    """The library's own puncturing tables (csrc/dab_tables.hpp, host code the device tables are built from), printed
    by a small program compiled against the header."""
    src = tmp_path / "dump_masks.cpp"
    src.write_text("""
#include <cstdio>
#include "dab_tables.hpp"
static void put(const char *name, int a, int b, int c, const dab::PunctureProfile &p, int cu) {
    std::printf("%s %d %d %d %d %d ", name, a, b, c, p.nsteps, cu);
    for (uint8_t f : p.mask) std::putchar('0' + f);
    std::putchar('\\n');
}
int main() {
    for (int pi = 1; pi <= 24; pi++) {
        uint8_t v[32]; dab::puncture_vector(pi, v);
        std::printf("pi %d 0 0 8 0 ", pi);
        for (int i = 0; i < 32; i++) std::putchar('0' + v[i]);
        std::putchar('\\n');
    }
    put("fic", 0, 0, 0, dab::make_fic_profile(), 0);
    for (int type = 0; type < 2; type++)
        for (int level = 1; level <= 4; level++)
            for (int br = 8; br <= 1728; br += 8) {
                dab::PunctureProfile p; int cu = 0;
                if (dab::make_eep_profile(type, level, br, p, cu)) put("eep", type, level, br, p, cu);
            }
    for (int i = 0; i < 64; i++) {
        dab::PunctureProfile p; int cu = 0;
        if (dab::make_uep_profile(i, p, cu)) put("uep", i, 0, 0, p, cu);
    }
}
""")
    exe = tmp_path / "dump_masks"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "csrc"),
                           str(src), "-o", str(exe)])
    rows = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        name, a, b, c, nsteps, cu, bits = line.split()
        rows[(name, int(a), int(b), int(c))] = (int(nsteps), int(cu), np.frombuffer(bits.encode(), np.uint8) - 48)
    return rows


def test_reference_masks_equal_the_oracles_and_the_librarys(built, tmp_path):
    """An equality of tables, entry by entry, so that a disagreement names the entry: every puncturing vector, the
    FIC, every EEP profile the binding accepts (and the over-long ones the library decodes), all 64 UEP rows."""
    from oracle import oracle as O
    import dabgpu
    lib = _mask_dump(tmp_path)
    for pi in range(1, 25):
        assert (O.puncture_vector(pi) == R.V_PI[pi - 1]).all(), ("oracle", pi)
        assert (lib[("pi", pi, 0, 0)][2] == R.V_PI[pi - 1]).all(), ("library", pi)
    p = R.fic_profile()
    assert (O.fic_puncture_mask()[0] == p.mask).all() and (lib[("fic", 0, 0, 0)][2] == p.mask).all()
    assert p.mask[-24:].tolist() == R.V_TAIL.tolist()
    n_eep = 0
    for opt in (0, 1):
        for lvl in (1, 2, 3, 4):
            for br in range(8, 1729, 8):
                sc = dabgpu.Subchannel(0, 0, 0, opt, lvl, br)
                try:
                    p = R.eep_profile(opt, lvl, br)
                except ValueError:
                    assert ("eep", opt, lvl, br) not in lib, (opt, lvl, br)
                    continue
                sc.length = p.size_cu
                accepted = dabgpu.lib().dabgpu_subchannel_bytes(C.byref(sc)) == br * 3
                assert accepted == (p.size_cu <= 864) == (("eep", opt, lvl, br) in lib), (opt, lvl, br)
                if not accepted:
                    continue
                n_eep += 1
                ns, cu, m = lib[("eep", opt, lvl, br)]
                assert (ns, cu) == (p.nsteps, p.size_cu) and (m == p.mask).all(), ("library", opt, lvl, br)
                om, kept, ons, ocu = O.eep_puncture_mask(opt, lvl, br)
                assert (kept, ons, ocu) == (p.kept, p.nsteps, p.size_cu) and (om == p.mask).all(), ("oracle", opt, lvl, br)
    assert n_eep > 400
    for i in range(64):
        p = R.uep_profile(i)
        ns, cu, m = lib[("uep", i, 0, 0)]
        assert (ns, cu) == (p.nsteps, p.size_cu) and (m == p.mask).all(), ("library", i)
        om, kept, ons, ocu = O.uep_puncture_mask(i)
        assert (kept, ons, ocu) == (p.kept, p.nsteps, p.size_cu) and (om == p.mask).all(), ("oracle", i)
        sc = dabgpu.uep_subchannel(i, 0)
        assert sc.length == p.size_cu and sc.bitrate_kbps == p.bitrate


def _bit_level_rx(frame_bits, rng, noisy):
    soft = np.where(frame_bits > 0, 127, -127).astype(np.int64)
    if noisy:
        soft = np.clip(soft + rng.integers(-90, 91, soft.shape), -127, 127)
    return soft.astype(np.int8)


SYNTH_PROFILES = [("eep", 0, lv, 32) for lv in (1, 2, 3, 4)] + [("eep", 1, lv, 32) for lv in (1, 2, 3, 4)] + \
                 [("uep", i, 0, 0) for i in (0, 4, 15, 63)]


@pytest.mark.parametrize("kind,a,b,c", SYNTH_PROFILES)
def test_reference_returns_what_the_numpy_transmitter_sent(kind, a, b, c):
    """dabgpu/synth.py (an independent transmitter) -> fic_reference / msc_reference, byte for byte: noise-free and
    with the +-90 uniform noise test_uep.py uses, in one call and cut into calls with the history carried."""
    from dabgpu import synth
    n_frames = 5
    if kind == "eep":
        e = synth.Ensemble(seed=700 + 10 * a + b, n_frames=n_frames, option=a, level=b, bitrate=c, start_cu=7)
        p = R.eep_profile(a, b, c)
    else:
        start = 7 if a != 63 else 448
        e = synth.Ensemble(seed=800 + a, n_frames=n_frames, uep_index=a, start_cu=start)
        p = R.uep_profile(a)
    assert p.size_cu == e.size_cu and (p.mask == e.mask).all()
    rng = np.random.default_rng(a + b)
    for noisy in (False, True):
        soft = _bit_level_rx(e.frame_bits, rng, noisy)
        fic = R.fic_reference(soft)
        assert (fic.fib == e.fibs).all() and fic.crc_ok.all()
        assert (R.metric_of(fic.fib.reshape(-1, 96), fic.mother, dispersed=True) == fic.decoded.best).all()
        cifs = soft[:, synth.NB_FIC_BITS:].reshape(4 * n_frames, synth.NB_CIF_BITS)[:, 64 * e.start_cu:64 * (e.start_cu + p.size_cu)]
        whole = R.msc_reference(cifs, None, p)
        assert (whole.out[15:] == e.msc_bytes[:5]).all()                         # logical frame r is complete at CIF r + 15
        # the transmission is cyclic: with the last 15 CIFs as history every logical frame comes back
        again = R.msc_reference(cifs, cifs[-15:], p)
        assert (again.out == np.roll(e.msc_bytes, 15, axis=0)).all()
        # ... and cut into calls of 1, 4, 15 CIFs with the history handed on
        h, outs = cifs[-15:], []
        for lo, hi in ((0, 1), (1, 5), (5, 20)):
            r = R.msc_reference(cifs[lo:hi], h, p)
            h = r.history
            outs.append(r.out)
        assert (np.concatenate(outs) == again.out).all() and (h == cifs[-15:]).all()


def test_synth_interleaver_then_reference_deinterleaver_is_a_delay_of_15_cifs():
    from dabgpu import synth
    rng = np.random.default_rng(5)
    R_, nbits = 40, 16 * 37
    frames = rng.integers(-127, 128, (R_, nbits)).astype(np.int8)
    tx = synth.time_interleave(frames, cyclic=False)                             # [R][nbits], first CIFs partly zero
    out, hist = R.time_deinterleave(tx)
    assert (out[15:] == frames[:R_ - 15]).all() and (hist == tx[-15:]).all()
    assert (R.time_interleave(frames)[:R_] == tx).all()                          # the reference's own transmitter side
    h, parts = None, []
    for lo, hi in ((0, 1), (1, 16), (16, 32), (32, 40)):                         # 1, 15, 16 and 8 CIFs
        o, h = R.time_deinterleave(tx[lo:hi], h)
        parts.append(o)
    assert (np.concatenate(parts) == out).all()


# ================================================================================================ CPU: the families
def test_headroom_family_reaches_its_excursion():
    """The condition the headroom tests stand on, by the reference alone: the family reaches the excursion of a clean
    +-127 codeword of a random message (9 906 single units) and goes beyond it."""
    soft, fam = headroom_pool()
    _, d = headroom_ref()
    assert np.abs(soft.astype(np.int64)).max() == 127
    worst = {}
    for f, e, s in zip(fam, d.excursion, d.spread):
        worst[f] = (max(worst.get(f, (0, 0))[0], int(e)), max(worst.get(f, (0, 0))[1], int(s)))
    for f, (e, s) in worst.items():
        _report("headroom / %-34s excursion %5d (doubled %5d, %2d %% of 24 480)  spread %5d" % (f, e, 2 * e, round(100 * e / HEADER_BOUND), s))
    top = int(d.excursion.max())
    _report("headroom family: largest excursion %d single units = %d doubled" % (top, 2 * top))
    assert worst["clean, random message"][0] >= CLEAN_EXCURSION
    assert top == MAX_EXCURSION == CLEAN_EXCURSION                               # the largest there is: see max_excursion()
    g = np.load(golden_path("decoder_headroom.npz"))
    k = [i for i, f in enumerate(fam) if f.startswith("searched")]
    assert (d.excursion[k] == g["excursion"]).all() and (d.spread[k] == g["spread"]).all() and (d.best[k] == g["best"]).all()
    assert g["excursion"].min() == MAX_EXCURSION and g["excursion_of_start"].min() < MAX_EXCURSION
    # the header of viterbi_lane_kernels.hip argues that nothing exceeds 12 240: an input beyond it would be a finding
    assert top <= HEADER_BOUND, "an input exceeds the bound the lane kernel's header derives: %d" % top


def test_lures_are_lures():
    soft, fam = lure_pool()
    _, d = lure_ref()
    full = 4 * 127 * NSTEPS_H
    for i, f in enumerate(fam):
        if not f.startswith("both"):
            assert soft[i].astype(np.int64).__abs__().sum() == full
            assert d.best[i] < full, f                   # a path outside the known start / end state explains it better
    _report("lures: the forbidden path leads by %d .. %d" % (int((full - d.best[:]).min()), int((full - d.best).max())))


def test_signal_families_have_unique_optima():
    """At least 90 % of the signal-plus-noise codewords (4, 8, 12, 20 dB) of the long-codeword family have one optimum
    only, by the reference alone: there, equal bytes follow from maximum likelihood whatever the tie rule.  Measured
    per case and printed.  With PI 24 and the real masks every signal codeword is unique.  With PI 1 (rate 8/9) every
    codeword at 8 dB and above is, but at 4 dB the decoder is past its limit, error events follow one another and
    some end in an exact tie: 7 of 12 codewords of 3 078 steps and 0 of 6 of 27 654 steps are unique at amplitude
    127, and no amplitude changes that (40, 60, 90 were tried: 2 .. 4 of 12, 0 of 6).  The 90 % therefore holds for
    the family as a whole, and case by case from 8 dB on, where it is asserted as 100 %."""
    total = unique = 0
    for nsteps in LONG_LENGTHS:
        for kind in LONG_KINDS:
            _, _, kinds = long_case(nsteps, kind)
            _, d = long_ref(nsteps, kind)
            sig = np.array([k.endswith("dB") for k in kinds])
            above = np.array([k.endswith("dB") and k != "4dB" for k in kinds])
            _report("long %5d steps / %-4s: unique optimum on %2d of %2d signal codewords (amplitude %d), %d of %d at 4 dB; excursion %5d"
                    % (nsteps, kind, int(d.unique[sig].sum()), int(sig.sum()), AMPLITUDE[kind], int(d.unique[sig & ~above].sum()),
                       int((sig & ~above).sum()), int(d.excursion.max())))
            assert d.unique[above].all(), (nsteps, kind)
            if kind != "pi1":
                assert d.unique[sig].all(), (nsteps, kind)
            total += int(sig.sum())
            unique += int(d.unique[sig].sum())
            zeros = kinds.index("zeros")
            assert not d.unique[zeros] and d.best[zeros] == 0 and not d.bits()[zeros].any() and d.bits(R.OPPOSITE)[zeros].any()
    _report("long codewords, signal plus noise: unique optimum on %d of %d" % (unique, total))
    assert unique >= 0.9 * total
    for kind in MSC_TYPES:
        u = np.concatenate([r.decoded.unique for r in msc_ref(kind)])
        e = max(int(r.decoded.excursion.max()) for r in msc_ref(kind))
        _report("msc %-5s: unique optimum on %d of %d codewords; excursion %d" % (kind, int(u.sum()), u.size, e))
        assert u[15:196].mean() >= 0.9                   # (before CIF 15 parts of the codeword are erased)
    f = fic_ref().decoded
    _report("fic: unique optimum on %d of %d codewords; excursion %d" % (int(f.unique.sum()), f.unique.size, int(f.excursion.max())))
    assert f.unique[:20].all()


# ================================================================================================ CPU: the oracle
_assert_decoder = R.assert_decoder                       # (shared with test_decoder_profiles.py)


def _oracle_plain(mother):
    from oracle import oracle as O
    return np.stack([np.packbits(O.viterbi(m.astype(np.int8))) for m in mother])


@pytest.mark.parametrize("nsteps", LONG_LENGTHS)
def test_oracle_on_the_long_codewords(built, nsteps):
    for kind in LONG_KINDS:
        mother, d = long_ref(nsteps, kind)
        _assert_decoder(_oracle_plain(mother), mother, d, False, "oracle, %d steps, %s" % (nsteps, kind))


def test_oracle_on_headroom_and_lures(built):
    """(The place a flaw in the oracle's -8192 start penalty would show without a GPU.)"""
    for name, (mother, d) in (("headroom", headroom_ref()), ("lures", lure_ref())):
        _assert_decoder(_oracle_plain(mother), mother, d, False, "oracle, " + name)


def test_oracle_on_the_fic_and_msc_cases(built):
    from oracle import oracle as O
    soft, fibs, flags = fic_case()
    ref = fic_ref()
    assert (ref.fib[:3] == fibs).all() and (ref.crc_ok[:3] == flags).all()      # saturated: returned as sent
    got = [O.fic_decode(s) for s in soft]
    _assert_decoder(np.stack([g[0] for g in got]).reshape(-1, 96), ref.mother, ref.decoded, True, "oracle, FIC")
    assert (np.stack([g[1] for g in got]) == ref.crc_ok).all()
    for kind in MSC_TYPES:
        p = msc_profile(kind)
        sub, data = msc_case(kind)
        for s, r in enumerate(msc_ref(kind)):
            if s == 0:
                assert (r.out[15:] == data[s]).all(), kind                       # saturated: what was sent comes back
            rows = np.concatenate([np.zeros((15, sub.shape[2]), np.int8), sub[s]])
            got = np.stack([O.msc_decode_lf(O.time_deinterleave(rows[t:t + 16])[:p.kept], p.mask, p.nsteps) for t in range(sub.shape[1])])
            _assert_decoder(got, r.mother, r.decoded, True, "oracle, MSC %s stream %d" % (kind, s))
            assert (r.history == sub[s, -15:]).all()


# ================================================================================================ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("nsteps", LONG_LENGTHS)
@pytest.mark.parametrize("kind", LONG_KINDS)
def test_gpu_long_codewords(ctx, nsteps, kind):
    mask, punct, _ = long_case(nsteps, kind)
    mother, d = long_ref(nsteps, kind)
    _assert_decoder(ctx.viterbi(punct, mask), mother, d, False, "viterbi, %d steps, %s" % (nsteps, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 24576 + 65])
def test_gpu_headroom_at_the_lane_kernels_batch_shapes(ctx, n):
    """Saturated inputs whose path metrics go as far from the renormalisation reference as inputs can (see
    test_headroom_family_reaches_its_excursion), one per lane, at 1, 63, 64, 65, 257 codewords and above the
    launcher's switch-over to the lane kernels (24 576)."""
    soft, _ = headroom_pool()
    mother, d = headroom_ref()
    mask = np.ones(4 * NSTEPS_H, np.uint8)
    pick = np.arange(n) % 257                            # 257 is prime to 64: the lanes of a group all differ
    got = ctx.viterbi(soft[pick], mask)
    if n <= 257:
        sub = d.lanes(pick)
        _assert_decoder(got, mother[pick], sub, False, "headroom, %d codewords" % n)
    else:
        assert (got == got[pick]).all(), "equal inputs, different lanes, different bytes"
        sub = d.lanes(np.arange(257))
        _assert_decoder(got[:257], mother[:257], sub, False, "headroom, first 257 of %d codewords" % n)
        _assert_decoder(got[n - 257:][np.argsort(pick[n - 257:])], mother[:257], sub, False, "headroom, last 257 of %d codewords" % n)


@pytest.mark.gpu
def test_gpu_start_and_end_state_lures(ctx):
    soft, _ = lure_pool()
    mother, d = lure_ref()
    _assert_decoder(ctx.viterbi(soft, np.ones(4 * NSTEPS_H, np.uint8)), mother, d, False, "lures")


@pytest.mark.gpu
def test_gpu_fic_bytes_and_crc_flags(ctx):
    soft, fibs, flags = fic_case()
    ref = fic_ref()
    fib, ok = ctx.fic_decode(soft)
    _assert_decoder(fib.reshape(-1, 96), ref.mother, ref.decoded, True, "FIC")
    assert (ok == ref.crc_ok).all()
    assert (fib[:3] == fibs).all() and (ok[:3] == flags).all()


def _msc_streamed(c, layout, grouped):
    """Decode the two 49-frame streams in calls of 1, 15, 16 and 17 frames (a call takes whole frames: 4, 60, 64 and
    68 CIFs), the first with history = NULL, the history handed from call to call.  -> per type [2][196][bytes], the
    last histories, and (grouped) fib, crc_ok."""
    import dabgpu
    frames = msc_frames(layout).reshape(2, MSC_FRAMES, 230400)
    scs = [dabgpu.subchannel(MSC_STARTS[layout][0], 32, level=3, eep_type=0), dabgpu.subchannel(MSC_STARTS[layout][1], 32, level=4, eep_type=1),
           dabgpu.uep_subchannel(4, MSC_STARTS[layout][2])]
    outs, hist = [[] for _ in scs], [None] * 3
    fibs, oks = [], []
    lo = 0
    for n in MSC_CUTS:
        part = np.ascontiguousarray(frames[:, lo:lo + n].reshape(2 * n, 230400))
        lo += n
        if grouped:
            fib, ok, o, h = c.decode_frames(part, 2, scs, history_in=None if hist[0] is None else hist, want_history=True)
            fibs.append(fib.reshape(2, n, 12, 32)); oks.append(ok.reshape(2, n, 12))
            for i in range(3):
                outs[i].append(o[i]); hist[i] = h[i]
        else:
            for i, sc in enumerate(scs):
                o, h = c.msc_decode(sc, part, 2, history_in=hist[i], want_history=True)
                outs[i].append(o); hist[i] = h
    assert lo == MSC_FRAMES
    outs = [np.concatenate(o, axis=1) for o in outs]
    if grouped:
        return outs, hist, np.concatenate(fibs, axis=1), np.concatenate(oks, axis=1)
    return outs, hist, None, None


def _assert_msc(outs, hist, what):
    for i, kind in enumerate(MSC_TYPES):
        sub, _ = msc_case(kind)
        for s, r in enumerate(msc_ref(kind)):
            _assert_decoder(outs[i][s], r.mother, r.decoded, True, "%s, MSC %s stream %d" % (what, kind, s))
            assert (hist[i][s] == sub[s, -15:]).all(), (what, kind, s)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_gpu_msc_streams_cut_into_calls(ctx, layout):
    """EEP-A, EEP-B and UEP sub-channels at start address 0, an odd capacity unit and the last that fits, against
    msc_reference over the UNCUT stream."""
    outs, hist, _, _ = _msc_streamed(ctx, layout, False)
    _assert_msc(outs, hist, "msc_decode, layout %d" % layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_gpu_msc_lane_kernels_with_the_prep_kernel(built, layout):
    c = make_ctx(1, unfused=True)
    try:
        outs, hist, _, _ = _msc_streamed(c, layout, False)
    finally:
        c.close()
    _assert_msc(outs, hist, "unfused lane kernels, layout %d" % layout)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, None])
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_gpu_decode_frames_grouped_launch(built, layout, mode):
    """dabgpu_decode_frames (decode_frames_dev on the device): the FIC and the three sub-channels in one call; with
    the lane kernels the 16-frame call is one grouped launch of entries of different length."""
    c = make_ctx(mode)
    try:
        outs, hist, fib, ok = _msc_streamed(c, layout, True)
    finally:
        c.close()
    _assert_msc(outs, hist, "decode_frames, layout %d" % layout)
    ref = msc_fic_ref(layout)
    _assert_decoder(fib.reshape(-1, 96), ref.mother, ref.decoded, True, "decode_frames, FIC, layout %d" % layout)
    assert (ok.reshape(-1, 12) == ref.crc_ok).all()
