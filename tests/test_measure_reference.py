"""The measurement calls -- dabgpu_tii_frames_dev / _acquired_dev, dabgpu_cir_frames_dev / _acquired_dev, dabgpu_mer_dev,
dabgpu_channel_ber_dev -- against tests/tii_reference.py, tests/cir_reference.py (float64, with the per-element budgets
derived in their docstrings) and tests/quality_reference.py (integers, exact).

The CPU part holds the references to known answers, shows that no budget is wider than the 1e-4-of-the-maximum bars of
test_tii.py / test_cir.py and that a float32 restatement of the same operations stays inside every budget on every GPU
case (so the budgets can be met), and that each mutant of the references listed in MUTANTS leaves its budget somewhere
(so the budgets can see the errors the features exist to report).  The GPU part compares every element of every record
with its budget, and bit for bit wherever the result is a sum, a count or a copy."""
import functools
import math

import numpy as np
import pytest

import dabgpu
from dabgpu import synth
from conftest import make_ctx
import cir_reference as CR
import decoder_reference as DR
import ofdm_reference as OR
import quality_reference as QR
import tii_reference as TR

NFFT, NULL, SYM = 2048, 2656, 2552
EXT = NFFT + 2                                     # a case carries the sample before and the sample after each window
SCALE2 = NFFT ** 2 / 1536                          # power of one unit carrier in an unnormalised FFT bin
CARRIER = 1.0 / 2048
STEP = 2.0 ** -32
# 0, dphi = +-1, +-0.37, +-5.2 and +-200 carriers, half a cycle per sample, the two ties of the phase-step rounding
# (0.5 -> 0 and 1.5 -> 2 steps: ties to even)
OFFSETS = np.array([0.0, STEP, -STEP, 0.37 * CARRIER, -0.37 * CARRIER, 5.2 * CARRIER, -5.2 * CARRIER, 200 * CARRIER,
                    -200 * CARRIER, 0.5, 0.5 * STEP, 1.5 * STEP], np.float32)
FORMATS = {"cf32": (dabgpu.IQ_CF32, 8), "cs16": (dabgpu.IQ_CS16, 4), "cs8": (dabgpu.IQ_CS8, 2), "cu8": (dabgpu.IQ_CU8, 2)}
KINDS = {"tii": (dabgpu.TII_ACC_DTYPE, NULL, 37), "cir": (dabgpu.CIR_ACC_DTYPE, SYM, 38)}      # record, min stride, padding


# ------------------------------------------------------------------------------------------------------ inputs
def quantise(ext, fmt):
    """ext [n][EXT] complex128 -> (what the device gets, the values it denotes [n][EXT] complex128).  The integer formats
    are driven to full scale and hold both ends of their range."""
    if fmt == "cf32":
        raw = ext.astype(np.complex64)
        return raw, raw.astype(np.complex128)
    v = np.stack([ext.real, ext.imag], -1)
    peak = np.abs(v).max()
    if fmt == "cu8":
        q = np.clip(np.rint(v / peak * 127.5 + 127.5), 0, 255).astype(np.uint8)
        q[0, 5, 0], q[0, 6, 1], q[-1, 900, 0], q[-1, 901, 1] = 0, 255, 255, 0
        val = q.astype(np.float64) - 127.5
    else:
        dt, top = (np.int16, 32767) if fmt == "cs16" else (np.int8, 127)
        q = np.clip(np.rint(v / peak * (top + 0.5)), -top - 1, top).astype(dt)
        q[0, 5, 0], q[0, 6, 1], q[-1, 900, 0], q[-1, 901, 1] = -top - 1, top, top, -top - 1
        val = q.astype(np.float64)
    return q, val[..., 0] + 1j * val[..., 1]


class Case:
    def __init__(self, kind, name, ext, fo=None, fmt="cf32"):
        self.kind, self.name, self.fmt = kind, name, fmt
        self.raw, self.val = quantise(np.asarray(ext, np.complex128).reshape(-1, EXT), fmt)
        self.n = self.val.shape[0]
        self.fo = np.zeros(self.n, np.float32) if fo is None else np.asarray(fo, np.float32)
        assert self.fo.shape == (self.n,)

    @property
    def windows(self):
        return self.val[:, 1:1 + NFFT]

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """TII: (cells [n][24][8], floors [n], cell budgets, floor budgets); CIR: (taps [n][2048], carriers [n][1536],
        tap budgets, carrier budgets)."""
        rec = TR.record if self.kind == "tii" else CR.record
        return tuple(np.array(a) for a in zip(*[rec(w, f, budgets=True) for w, f in zip(self.windows, self.fo)]))


def white(rng, n, sigma2):
    return math.sqrt(sigma2 / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def tone_and_impulse():
    n = np.arange(EXT) - 1
    tone = np.exp(2j * np.pi * 300 * n / NFFT)
    imp = np.zeros(EXT, np.complex128)
    imp[700] = 1.0 + 0.5j
    return tone, imp


def tii_ext(rng, ids, n, snr_db):
    """n windows of the null symbol of transmitters `ids` (synth.tii_null), noise at snr_db per bin below a unit carrier."""
    base = synth.tii_null(ids).astype(np.complex128) if ids else np.zeros(NULL, np.complex128)
    out = []
    for _ in range(n):
        x = base.copy()
        if snr_db is not None:
            x += white(rng, NULL, SCALE2 / (NFFT * 10 ** (snr_db / 10)))
        out.append(x[NULL - TR.WIN_BEGIN - 1:NULL - TR.WIN_END + 1])
    return np.array(out)


@functools.lru_cache(maxsize=None)
def prs_symbol():
    """the 2552 samples of the PRS (prefix + useful part) at unit mean power"""
    Z = np.zeros(NFFT, np.complex128)
    Z[CR.BINS] = CR.prs() * (NFFT / math.sqrt(1536))
    u = np.fft.ifft(Z)
    return np.concatenate([u[-504:], u])


def cir_ext(rng, paths, n, snr_db):
    """n windows of a PRS through `paths` = [(delay, gain)] (delays may be negative: a pre-echo), noise at snr_db below
    the unit-power symbol."""
    lead = 16
    out = []
    for _ in range(n):
        x = np.zeros(lead + SYM + 1024, np.complex128)
        for d, g in paths:
            x[lead + d:lead + d + SYM] += g * prs_symbol()
        if snr_db is not None:
            x += white(rng, x.size, 10 ** (-snr_db / 10))
        out.append(x[lead + CR.WIN_BEGIN - 1:lead + CR.WIN_END + 1])
    return np.array(out)


@functools.lru_cache(maxsize=None)
def cases(kind):
    tone, imp = tone_and_impulse()
    if kind == "tii":
        rng = np.random.default_rng(0x711)
        c = [Case(kind, "noise", tii_ext(rng, [], 2, 0.0)),
             Case(kind, "zero", np.zeros((2, EXT)), fo=[0.0, 0.37 * CARRIER]),
             Case(kind, "tone", tone),
             Case(kind, "impulse", imp),
             Case(kind, "one_8dB", tii_ext(rng, [(4, 17)], 2, 8.0)),
             Case(kind, "three_0_20_40dB", tii_ext(rng, [(3, 10), (11, 45, 0.1), (19, 62, 0.01)], 2, 8.0)),
             Case(kind, "one_clean", tii_ext(rng, [(20, 3)], 1, None)),
             Case(kind, "offsets", tii_ext(rng, [(9, 60)], len(OFFSETS), 8.0), fo=OFFSETS),
             Case(kind, "tone_offsets", np.tile(tone, (2, 1)), fo=[200 * CARRIER, -200 * CARRIER])]
        for fmt in ("cs16", "cs8", "cu8"):
            c.append(Case(kind, fmt, tii_ext(rng, [(2, 9)], 2, 6.0), fo=[0.37 * CARRIER, 0.0], fmt=fmt))
        return c
    rng = np.random.default_rng(0xC12)
    c = [Case(kind, "noise", white(rng, 2 * EXT, 0.3)),
         Case(kind, "zero", np.zeros((2, EXT)), fo=[0.0, 0.37 * CARRIER]),
         Case(kind, "tone", tone),
         Case(kind, "impulse", imp),
         Case(kind, "flat", cir_ext(rng, [(0, 1.0)], 1, None)),
         Case(kind, "two_paths_15dB", cir_ext(rng, [(0, 1.0), (23, 0.5)], 2, 15.0)),
         Case(kind, "pre_echo", cir_ext(rng, [(0, 1.0), (-5, 0.5)], 1, 15.0)),
         Case(kind, "path_at_600", cir_ext(rng, [(0, 1.0), (600, 0.5)], 1, 15.0)),
         Case(kind, "minus_40dB_15dB", cir_ext(rng, [(0, 1.0), (100, 0.01)], 2, 15.0)),
         Case(kind, "minus_40dB_clean", cir_ext(rng, [(0, 1.0), (100, 0.01)], 1, None)),
         Case(kind, "offsets", cir_ext(rng, [(0, 1.0), (23, 0.5)], len(OFFSETS), 15.0), fo=OFFSETS),
         Case(kind, "tone_offsets", np.tile(tone, (2, 1)), fo=[200 * CARRIER, -200 * CARRIER])]
    for fmt in ("cs16", "cs8", "cu8"):
        c.append(Case(kind, fmt, cir_ext(rng, [(0, 1.0), (17, 0.4)], 2, 12.0), fo=[0.37 * CARRIER, 0.0], fmt=fmt))
    return c


def case_ids(kind):
    return [c.name for c in cases(kind)]


def ratio(got, want, budget):
    """|got - want| / budget per element; an element whose budget is 0 must be exact (inf where it is not)."""
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(budget > 0, d / np.where(budget > 0, budget, 1.0), np.where(d > 0, np.inf, 0.0))


WORST = {}                                         # quantity -> worst ratio seen by the tests that have run (printed)


def note(tag, quantity, r):
    worst = float(np.max(r))
    key = "%s %s" % (tag, quantity)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("%-8s %-12s worst ratio to budget %.3f (so far %.3f)" % (tag, quantity, worst, WORST[key]))
    return worst


# ------------------------------------------------------------------------------------------------------ CPU: known answers
def test_known_answers_of_the_float_references():
    """A unit path at delay d gives tap[d] = 1 and unit carriers; one transmitter fills exactly its 32 carriers; and each
    budget at these elements is a few 1e-6 of the value."""
    for d in (0, 7, 213):
        ext = cir_ext(None, [(d, 1.0)], 1, None)[0]
        tap, car, tap_b, car_b = CR.record(ext[1:1 + NFFT], 0.0, budgets=True)
        assert abs(tap[d] - 1.0) < 1e-9 and tap.argmax() == d and np.all(np.abs(car - 1.0) < 1e-9)
        assert 0 < tap_b[d] < 2e-6 and np.all(car_b < 2e-5) and np.all(car_b > 0)
    for c, p in ((0, 0), (23, 69), (11, 37)):
        ext = tii_ext(None, [(c, p)], 1, None)[0]
        X, e = TR.spectrum(ext[1:1 + NFFT])
        P = np.abs(X) ** 2
        on = sorted(int(k) for k in np.flatnonzero(P > 1e-6 * SCALE2))
        assert on == sorted(k % NFFT for k in TR.transmitter_carriers(c, p)) and len(on) == 32
        assert np.all(np.abs(P[on] - SCALE2) < 1e-5 * SCALE2)             # (synth.tii_null rounds to complex64)
        cells, floor, cell_b, floor_b = TR.record(ext[1:1 + NFFT], budgets=True)
        want = np.zeros((24, 8))
        want[c, TR.positions(p)] = 8 * SCALE2
        assert np.all(np.abs(cells - want) < 1e-4 * SCALE2) and floor < 1e-12 * SCALE2
        assert np.all(cell_b[c, TR.positions(p)] < 1e-5 * 8 * SCALE2)
    # the correction is the 32-bit phase step of the float32 offset, from the window's first sample, in both references
    for f in OFFSETS:
        y = CR.correct(np.ones(NFFT), f)
        assert np.abs(y - OR.nco(NFFT, OR.dphi_of(f))).max() < 1e-12
        assert CR.phase_step(f) == OR.dphi_of(f)
    assert OR.dphi_of(0.5 * STEP) == 0 and OR.dphi_of(1.5 * STEP) == 2 and OR.dphi_of(-STEP) == 0xFFFFFFFF
    assert TR.C_NCO_DIRECT <= OR.C_NCO


def test_known_answers_of_the_exact_reference():
    """MER sums and BER counts counted by hand."""
    soft = np.zeros((1, QR.NB_FRAME_BITS), np.int8)
    sym = soft.reshape(1, 75, 3072)
    sym[0, 0, 0], sym[0, 0, 1536] = 127, -127                     # (a+b)^2 = 64516, (a-b)^2 = 0
    sym[0, 0, 1], sym[0, 0, 1537] = -128, 0                       # 16384, 16384
    sym[0, 0, 3], sym[0, 0, 1539] = 3, -4                         # 49, 1       (carrier 2 is (0, 0): not counted)
    sym[0, 74, 1535], sym[0, 74, 3071] = 0, -128                  # 16384, 16384
    s, e, n = QR.mer(soft)
    assert (int(s[0]), int(e[0]), int(n[0])) == (64516 + 16384 + 49 + 16384, 16384 + 1 + 16384, 4)
    s, e, n = QR.mer(soft, 0, 1)
    assert (int(s[0]), int(e[0]), int(n[0])) == (64516 + 16384 + 49, 16384 + 1, 3)
    s, e, n = QR.mer(soft, 1, 73)
    assert (int(s[0]), int(e[0]), int(n[0])) == (0, 0, 0)
    # FIC: decoded bytes that scramble to all zeros encode to all zeros
    zeros = np.packbits(DR.prbs(768))
    fib = np.tile(zeros, (1, 4, 1)).reshape(1, 12, 32)
    soft = np.full((1, 9216), -1, np.int8)
    e, b = QR.fic_ber(soft, fib)
    assert (e == 0).all() and (b == 2304).all()
    soft[0, 2304 + np.array([0, 17, 500, 2000, 2303])] = 1        # five wrong signs in codeword 1
    soft[0, 2 * 2304 + np.arange(7)] = 0                          # seven erasures in codeword 2
    e, b = QR.fic_ber(soft, fib)
    assert e[0].tolist() == [0, 5, 0, 0] and b[0].tolist() == [2304, 2304, 2297, 2304]
    # one information bit: the generators' weights 5 + 5 + 4 + 5, of which PI 16 keeps the first three of a step
    one = zeros.copy()
    one[0] ^= 0x80
    fib[0, 9:12] = one.reshape(3, 32)
    e, b = QR.fic_ber(np.full((1, 9216), -1, np.int8), fib)
    assert e[0].tolist() == [0, 0, 0, 14] and (b == 2304).all()
    # MSC without history: codeword t holds the bits whose delay d = bitrev4(i mod 16) reaches t + d >= 15: (t + 1) of 16
    p = DR.eep_profile(0, 3, 8)
    assert p.kept == 384 and p.size_cu == 6
    soft = np.zeros((1, QR.NB_FRAME_BITS), np.int8)
    soft[0, 9216:] = 1                                            # every decision 1, every coded bit 0
    dec = np.tile(np.packbits(DR.prbs(192)), (4, 1))
    e, b = QR.msc_ber(soft, 858, p, dec)
    assert e.tolist() == [24, 48, 72, 96] and b.tolist() == [24, 48, 72, 96]
    e, b = QR.msc_ber(soft, 858, p, dec, np.full((15, 384), -1, np.int8))
    assert e.tolist() == [24, 48, 72, 96] and b.tolist() == [384] * 4


# ------------------------------------------------------------------------------------------------------ CPU: satisfiable
def f32_spectrum(window, f):
    """A float32 restatement of the corrected transform: complex64 samples, float32 products, a complex64 FFT."""
    import torch
    x = np.asarray(window).astype(np.complex64)
    dphi = OR.dphi_of(f)
    if dphi:
        w = OR.nco(NFFT, dphi).astype(np.complex64)
        x = ((w.real * x.real - w.imag * x.imag) + 1j * (w.imag * x.real + w.real * x.imag)).astype(np.complex64)
    X = torch.fft.fft(torch.from_numpy(x)).numpy()
    assert X.dtype == np.complex64
    return X


def f32_power(X):
    return (X.real * X.real + X.imag * X.imag).astype(np.float32)


def f32_tii(window, f):
    P = f32_power(f32_spectrum(window, f))
    cells = np.zeros((24, 8), np.float32)
    for i in range(8):
        cells += P[TR.CELL_BINS[:, :, i]]
    floor = np.float32(P[TR.noise_bins()].sum(dtype=np.float32) / np.float32(304))
    return cells, floor


def f32_cir(window, f):
    import torch
    X = f32_spectrum(window, f)[CR.BINS]
    car = np.float32(1536 / NFFT ** 2) * f32_power(X)
    arg = CR.K.astype(np.float32) * np.float32(1.0 / 769.0)
    hann = (np.float32(0.5) * np.cos(np.pi * arg.astype(np.float64)).astype(np.float32) + np.float32(0.5)).astype(np.float32)
    w = (np.float32(math.sqrt(1536) / (NFFT * 768.0)) * hann).astype(np.float32)
    R = np.rint(CR.prs().real) + 1j * np.rint(CR.prs().imag)                  # a fourth root of unity, exactly
    assert np.abs(R - CR.prs()).max() < 1e-12
    c = (X.astype(np.complex128) * np.conj(R)).astype(np.complex64)          # swaps and negations: exact
    Y = np.zeros(NFFT, np.complex64)
    Y[CR.BINS] = (w * c.real + 1j * (w * c.imag)).astype(np.complex64)
    h = torch.fft.fft(torch.from_numpy(np.conj(Y))).numpy()
    return f32_power(h), car


@pytest.mark.parametrize("kind", ["tii", "cir"])
def test_budgets_are_under_the_old_bars_and_a_float32_restatement_is_inside_them(kind):
    """On every GPU case: no budget exceeds the bar test_tii.py / test_cir.py used -- 1e-4 of the largest cell, tap or
    carrier of the record, and 1e-4 of the floor for the floor (where there is no noise and the floor is below 1e-6 of a
    cell's share of the largest cell, a bar no arithmetic meets, 1e-4 of that share) -- and float32 arithmetic meets
    every budget."""
    names = ("cell", "floor") if kind == "tii" else ("tap", "carrier")
    share, inside = {n: 0.0 for n in names}, {n: 0.0 for n in names}
    for case in cases(kind):
        a, b, a_bud, b_bud = case.reference()
        for i in range(case.n):
            ga, gb = (f32_tii if kind == "tii" else f32_cir)(case.windows[i], case.fo[i])
            bars = (1e-4 * a[i].max(), 1e-4 * (b[i] if b[i] > 1e-6 * a[i].max() / 8 else a[i].max() / 8) if kind == "tii" else 1e-4 * b[i].max())
            for n, want, bud, got, bar in zip(names, (a[i], b[i]), (a_bud[i], b_bud[i]), (ga, gb), bars):
                assert np.all(bud <= bar), (case.name, i, n, float(np.max(bud)), bar)
                assert np.all(bud >= 0) and np.all(np.isfinite(bud))
                if bar > 0:
                    share[n] = max(share[n], float(np.max(bud)) / bar)
                r = float(np.max(ratio(got, want, bud)))
                inside[n] = max(inside[n], r)
                assert r <= 1.0, (case.name, i, n, r)
    for n in names:
        print("%s %-8s largest budget = %.4f of the old bar; float32 restatement at %.3f of its budget" % (kind, n, share[n], inside[n]))


# ------------------------------------------------------------------------------------------------------ CPU: sensitive
def cir_variant(ext, f, den=769.0, S=768.0, shift=0, seam=False, bin_err=None, weak=None):
    """cir_reference.record restated with one knob per mutant (the defaults give the reference)."""
    X = np.fft.fft(CR.correct(ext[1 + shift:1 + shift + NFFT], f))
    if bin_err is not None:
        X[bin_err] *= 1.0 + 1e-4
    Y = np.zeros(NFFT, np.complex128)
    Y[CR.BINS] = (0.5 + 0.5 * np.cos(np.pi * CR.K / den)) * X[CR.BINS] * np.conj(CR.prs())
    tap = np.abs(math.sqrt(1536) / (NFFT * S) * np.fft.ifft(Y) * NFFT) ** 2
    if weak is not None:
        tap = np.where(tap < 1e-4 * tap.max(), tap * weak, tap)
    k = np.concatenate([np.arange(-767, 1), np.arange(1, 769)]) if seam else CR.K
    return tap, 1536 / NFFT ** 2 * np.abs(X[k % NFFT]) ** 2


def tii_variant(ext, f, lo=776, hi=927, pair=1, shift=0, weak=None, sign=1.0):
    """tii_reference.record restated with one knob per mutant (the defaults give the reference)."""
    X, _ = TR.spectrum(ext[1 + shift:1 + shift + NFFT], np.float32(sign) * np.float32(f))
    P = np.abs(X) ** 2
    cells = np.zeros((24, 8))
    for c in range(24):
        for b in range(8):
            cells[c, b] = sum(P[(B + 2 * c + 48 * b) % NFFT] + P[(B + 2 * c + 48 * b + pair) % NFFT] for B in TR.BASES)
    if weak is not None:
        i = np.unravel_index(np.argmin(cells), cells.shape)
        cells[i] *= weak
    k = np.arange(lo, hi + 1)
    return cells, P[np.concatenate([k, NFFT - k])].mean()


MUTANTS = {
    "cir": [("weak taps x 1.01", dict(weak=1.01)), ("taper over 768", dict(den=768.0)), ("taper over 770", dict(den=770.0)),
            ("scale with S = 769", dict(S=769.0)), ("window one sample late", dict(shift=1)),
            ("carrier seam shifted", dict(seam=True)), ("one bin off by 1e-4", dict(bin_err=int(CR.BINS[100])))],
    "tii": [("floor over 776..926", dict(hi=926)), ("floor over 777..927", dict(lo=777)), ("cell takes k and k + 2", dict(pair=2)),
            ("window one sample early", dict(shift=-1)), ("one weak cell x 1.001", dict(weak=1.001)),
            ("correction's sign flipped", dict(sign=-1.0))],
}


@pytest.mark.parametrize("kind", ["tii", "cir"])
def test_every_mutant_of_the_reference_leaves_its_budget(kind):
    variant = tii_variant if kind == "tii" else cir_variant
    worst = {name: 0.0 for name, _ in MUTANTS[kind]}
    for case in cases(kind):
        a, b, a_bud, b_bud = case.reference()
        for i in range(case.n):
            ga, gb = variant(case.val[i], case.fo[i])
            assert np.abs(ga - a[i]).max() <= 1e-12 * max(a[i].max(), 1e-300), case.name      # the restatement is the reference
            assert np.abs(gb - b[i]).max() <= 1e-12 * max(np.max(b[i]), 1e-300), case.name
            for name, kw in MUTANTS[kind]:
                ga, gb = variant(case.val[i], case.fo[i], **kw)
                r = max(float(np.max(ratio(ga, a[i], a_bud[i]))), float(np.max(ratio(gb, b[i], b_bud[i]))))
                worst[name] = max(worst[name], r)
    for name, r in worst.items():
        print("%s mutant %-28s worst ratio to budget %.3g" % (kind, name, r))
    assert all(r > 1.0 for r in worst.values()), worst


# ------------------------------------------------------------------------------------------------------ CPU: exact parts
def test_exact_reference_equals_the_older_restatements(built):
    """quality_reference against test_quality.py's np_mer / fic_counts / msc_counts (the oracle's de-interleaver, synth's
    encoder) where their domains overlap: whole frames, EEP sub-channels, a carried history."""
    import test_quality as TQ
    rng = np.random.default_rng(0x0A11)
    soft = rng.integers(-128, 128, (3, QR.NB_FRAME_BITS)).astype(np.int8)
    soft[rng.random(soft.shape) < 0.1] = 0
    for first, n in ((0, 75), (0, 3), (40, 7)):
        s, e, c = QR.mer(soft, first, n)
        old = TQ.np_mer(soft, first, n)
        assert (old["signal"] == s).all() and (old["error"] == e).all() and (old["carriers"] == c).all()
    fib = rng.integers(0, 256, (3, 12, 32)).astype(np.uint8)
    e, b = QR.fic_ber(soft, fib)
    old = TQ.fic_counts(soft, fib)
    assert (old["errors"] == e).all() and (old["bits"] == b).all() and e.sum() > 0
    for (opt, lvl, br), start in (((0, 3, 64), 0), ((1, 2, 32), 100)):
        p = DR.eep_profile(opt, lvl, br)
        sc = dabgpu.subchannel(start, br, level=lvl, eep_type=opt)
        assert sc.length == p.size_cu
        dec = rng.integers(0, 256, (12, p.nbytes)).astype(np.uint8)
        for hist in (None, rng.integers(-128, 128, (15, 64 * p.size_cu)).astype(np.int8)):
            e, b = QR.msc_ber(soft, start, p, dec, hist)
            old = TQ.msc_counts(soft, sc, p.mask, dec, hist)
            assert (old["errors"] == e).all() and (old["bits"] == b).all() and e.sum() > 0


# ------------------------------------------------------------------------------------------------------ GPU helpers
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def records(kind, n, fill=0, init=None):
    import torch
    size = KINDS[kind][0].itemsize
    if init is not None:
        return dev(np.ascontiguousarray(init).view(np.uint8).reshape(n, size))
    t = torch.zeros((n, size), dtype=torch.uint8, device="cuda:0")
    return t.fill_(fill) if fill else t


def host(kind, t):
    return t.cpu().numpy().view(KINDS[kind][0]).reshape(-1)


def layout(kind, raw, stride, tail=0):
    """The windows raw [n][EXT] (one sample before, the window, one after) as frames `stride` samples apart -> (buffer,
    sample index of frame 0's PRS prefix).  TII: the window ends 304 samples before the prefix; CIR: it starts 504
    samples after it.  The samples between the windows stay zero."""
    n = raw.shape[0]
    first = TR.WIN_BEGIN + 1 if kind == "tii" else 0
    at = first - TR.WIN_BEGIN - 1 if kind == "tii" else CR.WIN_BEGIN - 1
    buf = np.zeros(((n - 1) * stride + at + EXT + tail,) + raw.shape[2:], raw.dtype)
    for i in range(n):
        buf[at + i * stride:at + i * stride + EXT] = raw[i]
    return buf, first


def frames_call(c, kind, d_buf, first, fmt, stride, S, F, fo, acc, frame):
    fn = c.tii_frames_dev if kind == "tii" else c.cir_frames_dev
    d_fo = None if fo is None else dev(np.asarray(fo, np.float32))
    fn(d_buf.data_ptr() + first * FORMATS[fmt][1], stride, S, F, acc.data_ptr(), d_freq_offset=None if fo is None else d_fo.data_ptr(),
       d_frame=None if frame is None else frame.data_ptr())
    c.sync()
    return d_fo


def sequential_sum(kind, rec, S, F, start=None):
    """what an accumulator holds after a call: the float32 frame-order sum of the records on top of `start`"""
    want = np.zeros(S, KINDS[kind][0]) if start is None else start.copy()
    fields = ("cell", "floor") if kind == "tii" else ("tap", "carrier")
    for s in range(S):
        for f in range(F):
            for name in fields:
                want[s][name] = want[s][name] + rec[s * F + f][name]          # float32 + float32, rounded once
            want[s]["frames"] += rec[s * F + f]["frames"]
    return want


def same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()


def check_records(case, rec, tag="MI355X"):
    """every element of every record of a case against its budget"""
    a, b, a_bud, b_bud = case.reference()
    names = ("cell", "floor") if case.kind == "tii" else ("tap", "carrier")
    assert (rec["frames"] == 1).all() and (rec["reserved"] == 0).all()
    worst = []
    for n, want, bud in zip(names, (a, b), (a_bud, b_bud)):
        got = rec[n].astype(np.float64)
        assert np.all(np.isfinite(got)), (case.name, n)
        worst.append(note(tag + " " + case.kind, n, ratio(got, want, bud)))
    assert max(worst) <= 1.0, (case.kind, case.name, worst)


@pytest.fixture(scope="module")
def mctx(built):
    c = make_ctx()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------ GPU: TII and CIR
def case_params():
    return [pytest.param(kind, i, id="%s-%s" % (kind, name)) for kind in ("tii", "cir") for i, name in enumerate(case_ids(kind))]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,index", case_params())
def test_gpu_every_element_of_every_case_within_its_budget(mctx, kind, index):
    """Every case of the CPU part through the frame call (one stream, the smallest stride), corrections through
    d_freq_offset, every sample format; an all-zero window gives all-zero records, no identifier and no path."""
    case = cases(kind)[index]
    c = mctx
    try:
        c.set_iq_format(FORMATS[case.fmt][0])
        buf, first = layout(kind, case.raw, KINDS[kind][1])
        d = dev(buf)
        acc, frame = records(kind, 1), records(kind, case.n, fill=0xA5)
        keep = frames_call(c, kind, d, first, case.fmt, KINDS[kind][1], 1, case.n, case.fo, acc, frame)
        rec, a = host(kind, frame), host(kind, acc)
        check_records(case, rec)
        assert same_bits(a, sequential_sum(kind, rec, 1, case.n))
        if case.name == "zero":
            for name in (("cell", "floor") if kind == "tii" else ("tap", "carrier")):
                assert (np.ascontiguousarray(rec[name]).view(np.uint32) == 0).all(), name
            if kind == "tii":
                assert len(dabgpu.tii_decode(a[0])) == 0
            else:
                rep, paths = dabgpu.cir_analyse(a[0])
                assert rep["n_paths"] == 0 and len(paths) == 0 and rep["peak"] == 0.0 and rep["floor"] == 0.0
        del keep
    finally:
        c.set_iq_format(dabgpu.IQ_CF32)


def pool(kind, n):
    """n noisy windows with a signal in them and corrections within +-3.5 carriers"""
    rng = np.random.default_rng(0x9001 + n)
    ext = tii_ext(rng, [(7, 33)], n, 8.0) if kind == "tii" else cir_ext(rng, [(0, 1.0), (23, 0.5)], n, 15.0)
    return Case(kind, "pool%d" % n, ext, fo=rng.uniform(-3.5, 3.5, n) * CARRIER)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tii", "cir"])
def test_gpu_shapes_strides_and_staged_records(built, kind):
    """streams x frames (1, 1), (3, 5), (2, 17) and (1, 1) again, at the smallest and at a padded stride: caller-owned
    records within their budgets, the sums their frame-order float32 sums; with d_frame == NULL (the context's own
    records, which grow between these calls: small, large, small) the sums are the same bits."""
    dt, min_stride, pad = KINDS[kind]
    c = make_ctx()
    try:
        for S, F in ((1, 1), (3, 5), (2, 17), (1, 1)):
            case = pool(kind, S * F)
            for stride in (min_stride, min_stride + pad):
                buf, first = layout(kind, case.raw, stride)
                d = dev(buf)
                staged = records(kind, S)
                k1 = frames_call(c, kind, d, first, "cf32", stride, S, F, case.fo, staged, None)
                acc, frame = records(kind, S), records(kind, S * F, fill=0xA5)
                k2 = frames_call(c, kind, d, first, "cf32", stride, S, F, case.fo, acc, frame)
                rec = host(kind, frame)
                check_records(case, rec)
                want = sequential_sum(kind, rec, S, F)
                assert same_bits(host(kind, acc), want), (S, F, stride)
                assert same_bits(host(kind, staged), want), (S, F, stride)
                del k1, k2
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tii", "cir"])
def test_gpu_corrections_through_the_stream_states(built, kind):
    """d_freq_offset == NULL: each of three streams is corrected by its own fine + coarse offset, added in float32."""
    S, F = 3, 2
    offs = [(0.3 * CARRIER, -3.0 * CARRIER), (-0.41 * CARRIER, 200.0 * CARRIER), (1.0e-7, -5.0 * CARRIER)]
    fo = np.repeat([OR.stream_correction(fine, coarse) for fine, coarse in offs], F).astype(np.float32)
    assert any(float(np.float32(a) + np.float32(b)) != float(np.float32(a)) + float(np.float32(b)) for a, b in offs)
    case = pool(kind, S * F)
    case = Case(kind, "states", case.val, fo=fo)
    c = make_ctx()
    try:
        c.streams_reset(S)
        for s, (fine, coarse) in enumerate(offs):
            c.set_stream_offsets(s, fine=fine, coarse=coarse)
        stride = KINDS[kind][1] + KINDS[kind][2]
        buf, first = layout(kind, case.raw, stride)
        d = dev(buf)
        acc, frame = records(kind, S), records(kind, S * F, fill=0xA5)
        frames_call(c, kind, d, first, "cf32", stride, S, F, None, acc, frame)
        rec = host(kind, frame)
        check_records(case, rec)
        assert same_bits(host(kind, acc), sequential_sum(kind, rec, S, F))
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tii", "cir"])
def test_gpu_scaled_copies_are_bit_identical(mctx, kind):
    """The input times 2^k, k = +-20: every record is the unscaled one times 4^k, bit for bit."""
    case = pool(kind, 3)
    stride = KINDS[kind][1]
    out = {}
    for k in (0, 20, -20):
        buf, first = layout(kind, (case.raw * np.float32(2.0 ** k)).astype(np.complex64), stride)
        d = dev(buf)
        acc, frame = records(kind, 1), records(kind, 3, fill=0xA5)
        keep = frames_call(mctx, kind, d, first, "cf32", stride, 1, 3, case.fo, acc, frame)
        out[k] = host(kind, frame).copy()
        del keep
    check_records(case, out[0])
    for k in (20, -20):
        for name in (("cell", "floor") if kind == "tii" else ("tap", "carrier")):
            assert same_bits(out[k][name], out[0][name] * np.float32(4.0 ** k)), (k, name)
            assert np.all(out[k][name] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tii", "cir"])
def test_gpu_accumulators_add_in_frame_order(mctx, kind):
    """1, 15, 16, 17 and 33 frames per stream (the accumulation kernels add in batches of 16 with a guarded tail), two
    streams, onto an accumulator that already holds sums, a frame count and reserved words: the sums are the sequential
    float32 sums bit for bit, the count exact, the reserved words untouched."""
    dt, stride, _ = KINDS[kind]
    rng = np.random.default_rng(0xACC)
    S = 2
    n_max = S * 33
    buf = white(rng, (n_max - 1) * stride + NULL + SYM, 1.0).astype(np.complex64)
    first = TR.WIN_BEGIN if kind == "tii" else 0
    d = dev(buf)
    zero = np.zeros(n_max, np.float32)
    for F in (1, 15, 16, 17, 33):
        start = np.zeros(S, dt)
        for name in (("cell", "floor") if kind == "tii" else ("tap", "carrier")):
            start[name] = rng.uniform(0.0, 1000.0, start[name].shape).astype(np.float32)
        start["frames"] = [7, 1 << 20]
        start["reserved"] = rng.integers(1, 1 << 30, start["reserved"].shape)
        acc, frame = records(kind, S, init=start), records(kind, S * F, fill=0xA5)
        keep = frames_call(mctx, kind, d, first, "cf32", stride, S, F, zero[:S * F], acc, frame)
        rec, a = host(kind, frame), host(kind, acc)
        assert (rec["frames"] == 1).all()
        want = sequential_sum(kind, rec, S, F, start)
        assert same_bits(a, want), F
        assert (a["frames"] == start["frames"] + F).all() and (a["reserved"] == start["reserved"]).all()
        del keep


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tii", "cir"])
@pytest.mark.parametrize("margin", [0, 504])
def test_gpu_acquired_slots_by_hand(mctx, kind, margin):
    """Hand-built slots of two streams behind a padded stream stride: flags 3 and 7 are counted, 0, 1 and 2 are not; a
    slot whose window (TII) or prefix (CIR) begins exactly at sample 0 of the capture is counted, one a sample earlier is
    not -- in the second stream that sample belongs to the first.  Counted slots equal the frame call's records on the
    same windows bit for bit, the others are all-zero records, and `frames` counts exactly the counted ones."""
    dt, stride, pad = KINDS[kind]
    rng = np.random.default_rng(0x510 + margin)
    S, F = 2, 6
    first = TR.WIN_BEGIN if kind == "tii" else 0                  # frame 0: the window / the prefix begins at sample 0
    per_stream = (F - 1) * stride + NULL + SYM
    stream_stride = per_stream + 2 * pad + 2
    x = white(rng, S * stream_stride, 1.0).astype(np.complex64)
    fo = (rng.uniform(-3.5, 3.5, S * F) * CARRIER).astype(np.float32)
    flags = np.array([[3, 7, 0, 1, 2, 3], [2, 3, 7, 3, 3, 0]], np.int32)
    slots = np.zeros((S, F), dabgpu.ACQUIRED_FRAME_DTYPE)
    slots["start"] = first + np.arange(F)[None, :] * stride - margin
    slots["freq_offset"] = fo.reshape(S, F)
    slots["flags"] = flags
    slots["start"][0, 5] = first - margin - 1                     # a sample before the capture
    slots["start"][1, 3] = first - margin - 1                     # a sample before the second stream's capture
    slots["start"][1, 4] = first - margin                         # exactly at its first sample (frame 0 of the stream)
    counted = (flags & 3) == 3
    counted[0, 5] = counted[1, 3] = False
    frame_of = np.tile(np.arange(F), (S, 1))
    frame_of[1, 4] = 0
    d = dev(x)
    d_slots = dev(slots.reshape(-1).view(np.uint8))
    acc, rec = records(kind, S), records(kind, S * F, fill=0x77)
    fn = mctx.tii_acquired_dev if kind == "tii" else mctx.cir_acquired_dev
    fn(d.data_ptr(), stream_stride, S, F, d_slots.data_ptr(), acc.data_ptr(), timing_margin=margin, d_frame=rec.data_ptr())
    mctx.sync()
    got, a = host(kind, rec).reshape(S, F), host(kind, acc)
    for s in range(S):
        want_fo = np.zeros(F, np.float32)                             # per frame: the offset of the slot that points at it
        for j in range(F):
            want_fo[frame_of[s, j]] = slots["freq_offset"][s, j]
        acc1, rec1 = records(kind, 1), records(kind, F, fill=0xA5)
        d_s = dev(x[s * stream_stride:(s + 1) * stream_stride])
        keep = frames_call(mctx, kind, d_s, first, "cf32", stride, 1, F, want_fo, acc1, rec1)
        ref = host(kind, rec1)
        for j in range(F):
            if counted[s, j]:
                i = frame_of[s, j]
                assert slots["freq_offset"][s, j] == want_fo[i]
                assert same_bits(got[s, j:j + 1], ref[i:i + 1]), (s, j)
            else:
                assert (got[s, j:j + 1].view(np.uint8) == 0).all(), (s, j)
        assert a[s]["frames"] == counted[s].sum()
        sel = got[s][counted[s]]
        assert same_bits(a[s:s + 1], sequential_sum(kind, sel, 1, len(sel))), s
        del keep
    assert counted.sum(axis=1).tolist() == [2, 3]


@pytest.mark.gpu
def test_gpu_cir_analysis_on_device_sums_equals_the_reference(mctx):
    """A path 40 dB down at 15 dB SNR, 32 frames: the library's analysis of the device's sums equals cir_reference.analyse
    on the same sums at range_db = 45, and with min_snr_db = 3 finds the weak path."""
    import test_cir as TC
    F = 32
    rng = np.random.default_rng(0x4045)
    case = Case("cir", "analyse", cir_ext(rng, [(0, 1.0), (100, 0.01)], F, 15.0))
    buf, first = layout("cir", case.raw, SYM)
    d = dev(buf)
    acc = records("cir", 1)
    keep = frames_call(mctx, "cir", d, first, "cf32", SYM, 1, F, case.fo, acc, None)
    a = host("cir", acc)[0]
    assert a["frames"] == F
    rep, got = TC.agree(a, F, range_db=45.0)
    assert [round(g[0]) for g in got] == [0]                      # (6 dB above the floor: under the default min_snr_db)
    rep, got = TC.agree(a, F, min_snr_db=3.0, range_db=45.0)
    assert [round(g[0]) for g in got] == [0, 100] and abs(got[1][1] + 40.0) < 1.5
    del keep


# ------------------------------------------------------------------------------------------------------ GPU: MER and BER
def random_soft(rng, n, stride=QR.NB_FRAME_BITS):
    """int8 over the whole range, -128 included, a tenth of the bytes zero and some carriers (0, 0)"""
    soft = rng.integers(-128, 128, (n, stride)).astype(np.int8)
    soft[rng.random(soft.shape) < 0.1] = 0
    sym = soft[:, :QR.NB_FRAME_BITS].reshape(n, 75, 3072).copy()
    erased = rng.random((n, 75, 1536)) < 0.05
    sym[..., :1536][erased] = 0
    sym[..., 1536:][erased] = 0
    sym[:, 0, 0], sym[:, 0, 1536] = -128, -128
    sym[:, 74, 1535], sym[:, 74, 3071] = -128, 127
    soft[:, :QR.NB_FRAME_BITS] = sym.reshape(n, -1)
    return soft


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames", [1, 4, 5, 7])
def test_gpu_mer_of_any_soft_bytes(mctx, n_frames):
    """Random int8 over the whole range (not what the quantiser writes): 1, 4, 5 and 7 frames (a workgroup holds four), the
    plain and a padded stride, four symbol ranges; the record behind the last one is not written."""
    import torch
    rng = np.random.default_rng(0x3E20 + n_frames)
    for stride in (QR.NB_FRAME_BITS, QR.NB_FRAME_BITS + 16):
        soft = random_soft(rng, n_frames, stride)
        d = dev(soft)
        for first, n in ((0, 75), (0, 1), (74, 1), (37, 38)):
            out = torch.full((n_frames + 1, 24), 0xA5, dtype=torch.uint8, device="cuda:0")
            mctx.mer_dev(d.data_ptr(), stride, n_frames, out.data_ptr(), first, n)
            mctx.sync()
            raw = out.cpu().numpy()
            got = raw[:n_frames].reshape(-1).view(dabgpu.MER_DTYPE)
            s, e, c = QR.mer(soft, first, n)
            assert (got["signal"] == s.astype(np.uint64)).all() and (got["error"] == e.astype(np.uint64)).all(), (stride, first, n)
            assert (got["carriers"] == c).all() and (got["reserved"] == 0).all() and c.min() > 0
            assert (raw[n_frames] == 0xA5).all()


class Sub:
    """a sub-channel of a BER call: the library's descriptor and the reference's profile of the same thing"""

    def __init__(self, start, eep=None, uep=None):
        self.start = start
        if uep is not None:
            self.sc, self.profile = dabgpu.uep_subchannel(uep, start), DR.uep_profile(uep)
        else:
            opt, lvl, br = eep
            self.sc, self.profile = dabgpu.subchannel(start, br, level=lvl, eep_type=opt), DR.eep_profile(opt, lvl, br)
        assert self.sc.length == self.profile.size_cu and self.sc.bitrate_kbps * 3 == self.profile.nbytes


def ber_call(c, d_soft, S, F, fib, subs, dec, hist):
    """one dabgpu_channel_ber_dev -> (fic counts [S F][4] or None, [counts [S][4 F] per sub-channel])"""
    import torch
    d_fib = None if fib is None else dev(fib)
    d_fic = torch.full((S * F, 4, 8), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_dec = [dev(x) for x in dec]
    d_hist = [None if h is None else dev(h) for h in hist]
    d_msc = [torch.full((S, 4 * F, 8), 0xA5, dtype=torch.uint8, device="cuda:0") for _ in subs]
    c.channel_ber_dev(d_soft.data_ptr(), QR.NB_FRAME_BITS, S, F, None if fib is None else d_fib.data_ptr(), d_fic.data_ptr(),
                      [u.sc for u in subs], None if all(h is None for h in d_hist) else [0 if h is None else h.data_ptr() for h in d_hist],
                      [x.data_ptr() for x in d_dec], [m.data_ptr() for m in d_msc])
    c.sync()
    fic = d_fic.cpu().numpy().reshape(-1).view(dabgpu.BER_DTYPE).reshape(S * F, 4)
    return (None if fib is None else fic), [m.cpu().numpy().reshape(-1).view(dabgpu.BER_DTYPE).reshape(S, 4 * F) for m in d_msc]


def ber_inputs(rng, S, F, subs, with_hist):
    dec = [rng.integers(0, 256, (S, 4 * F, u.profile.nbytes)).astype(np.uint8) for u in subs]
    hist = []
    for i, u in enumerate(subs):
        h = None
        if with_hist(i):
            h = rng.integers(-128, 128, (S, 15, 64 * u.profile.size_cu)).astype(np.int8)
            h[rng.random(h.shape) < 0.1] = 0
        hist.append(h)
    return dec, hist


def check_ber(soft, S, F, fib, fic, subs, dec, hist, msc):
    if fib is not None:
        e, b = QR.fic_ber(soft, fib)
        assert (fic["errors"] == e).all() and (fic["bits"] == b).all()
        assert e.min() > 0 and b.max() < 2304
    for i, u in enumerate(subs):
        for s in range(S):
            e, b = QR.msc_ber(soft[s * F:(s + 1) * F], u.start, u.profile, dec[i][s], None if hist[i] is None else hist[i][s])
            assert (msc[i][s]["errors"] == e).all() and (msc[i][s]["bits"] == b).all(), (i, s)
            assert e[-1] > 0 and b[-1] < u.profile.kept


@pytest.mark.gpu
def test_gpu_channel_ber_of_bytes_no_decoder_produced(mctx):
    """Random soft bytes with zeros sprinkled in, random "decoded" bytes: the FIC alone; then EEP-A at CU 0, EEP-B, a UEP
    row with padding bits and 1152 bytes per CIF ending at CU 864, two streams of three frames, with and without a
    carried history."""
    rng = np.random.default_rng(0xBE70)
    S, F = 2, 3
    soft = random_soft(rng, S * F)
    d_soft = dev(soft)
    fib = rng.integers(0, 256, (S * F, 12, 32)).astype(np.uint8)
    fic, _ = ber_call(mctx, d_soft, S, F, fib, [], [], [])
    check_ber(soft, S, F, fib, fic, [], [], [], [])
    subs = [Sub(0, eep=(0, 3, 64)), Sub(100, eep=(1, 2, 32)), Sub(200, uep=4), Sub(864 - 288, eep=(0, 3, 384))]
    assert subs[2].profile.padding > 0 and subs[3].profile.nbytes == 1152 and subs[3].start + subs[3].profile.size_cu == 864
    for with_hist in (lambda i: True, lambda i: False, lambda i: i % 2 == 0):
        dec, hist = ber_inputs(rng, S, F, subs, with_hist)
        fic, msc = ber_call(mctx, d_soft, S, F, fib, subs, dec, hist)
        check_ber(soft, S, F, fib, fic, subs, dec, hist, msc)
        _, alone = ber_call(mctx, d_soft, S, F, None, subs, dec, hist)
        for a, b in zip(alone, msc):
            assert (a == b).all()


@pytest.mark.gpu
def test_gpu_channel_ber_of_21_items_in_two_packs(mctx):
    """The FIC and 20 sub-channels of 8 kbit/s in one call (a launch holds 16 items: two launches), then the same 21
    items one call each: the reference's counts both times."""
    rng = np.random.default_rng(0xBE71)
    S, F = 1, 2
    soft = random_soft(rng, S * F)
    d_soft = dev(soft)
    fib = rng.integers(0, 256, (S * F, 12, 32)).astype(np.uint8)
    subs, start = [], 3
    for i in range(20):
        subs.append(Sub(start, eep=(0, 1 + i % 4, 8)))
        start += subs[-1].profile.size_cu + (i % 3)
    dec, hist = ber_inputs(rng, S, F, subs, lambda i: i % 3 != 1)
    fic, msc = ber_call(mctx, d_soft, S, F, fib, subs, dec, hist)
    check_ber(soft, S, F, fib, fic, subs, dec, hist, msc)
    fic1, _ = ber_call(mctx, d_soft, S, F, fib, [], [], [])
    assert (fic1 == fic).all()
    for i, u in enumerate(subs):
        _, one = ber_call(mctx, d_soft, S, F, None, [u], [dec[i]], [hist[i]])
        assert (one[0] == msc[i]).all(), i
