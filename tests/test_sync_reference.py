"""PRS synchronisation (dabgpu_sync_prs*) and acquisition (dabgpu_acquire*) against the float64 from-definition
reference tests/sync_reference.py.

Bars (derived in the reference's docstring): every integer choice -- k^, the tap, the first-path tap, each dip decision
-- lies in the reference's indistinguishable set, and equals the reference's exactly where that set holds one element;
ratios, fine and total frequency offsets within their budgets; threshold decisions exact outside their bands.  Every
group asserts how many of its cases were unambiguous (all signal cases at 8 dB and above must be).  The CPU tests check
the reference against the transmitted offsets and its direct sum against an FFT correlation, and run every case the GPU
tests use through the float32 oracle under the same bars."""
import functools

import numpy as np
import pytest

import sync_reference as SR
from dabgpu import synth

NULL = synth.NB_NULL
FRAME = synth.NB_FRAME_SAMPLES
SYMS = 76 * 2552
FMT_SCALE = {"cs16": 2000.0, "cs8": 25.0, "cu8": 25.0}

SYNC_DTYPE = np.dtype([("coarse_carriers", np.int32), ("time_offset", np.int32), ("peak_to_mean", np.float32),
                       ("coarse_peak_to_mean", np.float32)])


@functools.lru_cache(maxsize=None)
def _frame(seed):
    return synth.Ensemble(seed, n_frames=2).iq().ravel()


def quantise(x, fmt, scale=None):
    """complex -> (integer array [..., 2], complex128 values the reference and the oracle read)."""
    v = np.stack([x.real, x.imag], axis=-1).astype(np.float64)
    v *= (scale or FMT_SCALE[fmt]) / np.sqrt(np.mean(v * v))
    if fmt == "cs16":
        q = np.clip(np.rint(v), -32768, 32767).astype(np.int16)
        val = q.astype(np.float64)
    elif fmt == "cs8":
        q = np.clip(np.rint(v), -128, 127).astype(np.int8)
        val = q.astype(np.float64)
    else:
        q = np.clip(np.rint(v + 127.5), 0, 255).astype(np.uint8)
        val = q.astype(np.float64) - 127.5
    return q, val[..., 0] + 1j * val[..., 1]


# --------------------------------------------------------------------------------------------------- sync cases
def prs_window(cfo_carriers, early, snr, seed, correction=0.0):
    """2552 samples from `early` samples before the PRS prefix of a frame sent cfo_carriers high (and shifted so that
    the float32 correction `correction` is undone first).  Truth: t = early."""
    x = _frame(seed % 3)[:FRAME + 8192]
    st = NULL - early
    rng = np.random.default_rng(seed)
    seg = x[st - 64:st + 2552 + 64]
    rx = synth.channel(seg, snr_db=snr, cfo=cfo_carriers / 2048 - float(np.float32(correction)), rng=rng)
    return rx[64:64 + 2552]


class SyncCase:
    def __init__(self, name, windows, f=None, max_coarse=200, truth=None, fmt="cf32", stride=2552, snr=None,
                 signal=True, batch_D=False):
        self.name, self.fmt, self.stride, self.max_coarse = name, fmt, stride, max_coarse
        w = np.asarray(windows)
        if fmt == "cf32":
            self.q, self.values = w.astype(np.complex64), w.astype(np.complex64).astype(np.complex128)
        else:
            self.q, self.values = quantise(w, fmt)
        self.f = None if f is None else np.asarray(f, np.float32)
        self.truth = truth
        self.signal = signal and (snr is None or snr >= 8.0)
        D = None
        if batch_D:
            X = np.fft.fft(self.values[:, 504:2552], axis=1)
            D = SR.coarse_fft(np.roll(X, -1, axis=1) * np.conj(X), max_coarse)
        self.refs = [SR.Sync(v, 0.0 if self.f is None else self.f[i], max_coarse, D=None if D is None else D[i])
                     for i, v in enumerate(self.values)]


@functools.lru_cache(maxsize=None)
def sync_case(name):
    if name.startswith("coarse_"):
        M = int(name.split("_")[1])
        ks = sorted({0, 1, -1, M, -M} | ({M + 1, -(M + 1)} if M < 1023 else set()))
        w = [prs_window(k + 0.2, 100, 12.0, 10 + i) for i, k in enumerate(ks)]
        return SyncCase(name, w, None, M, truth=[(k, 100) if abs(k) <= M else (None, None) for k in ks], snr=12.0)
    if name == "fraction":
        fr = [0.2, 0.49, -0.49]
        w = [prs_window(5 + a, 37, 12.0, 20 + i) for i, a in enumerate(fr)]
        return SyncCase(name, w, None, 200, truth=[(int(np.rint(5 + a)), 37) for a in fr], snr=12.0)
    if name == "time":
        ts = [-1024, -1023, -504, -1, 0, 1, 503, 1023]
        w = [prs_window(3.2, t, 14.0, 30 + i) for i, t in enumerate(ts)]
        return SyncCase(name, w, None, 200, truth=[(3, t) for t in ts], snr=14.0)
    if name == "nco_wrap":
        fs = [0.5, -0.5, 0.4999, 0.37 / 2048]
        w = [prs_window(7.2, 64, 12.0, 40 + i, correction=f) for i, f in enumerate(fs)]
        return SyncCase(name, w, fs, 200, truth=[(7, 64)] * len(fs), snr=12.0)
    if name == "noise":
        rng = np.random.default_rng(50)
        w = (rng.standard_normal((6, 2552)) + 1j * rng.standard_normal((6, 2552))) * 0.7
        return SyncCase(name, w, None, 200, signal=False)
    if name == "scaled":
        base = prs_window(5.2, 100, 12.0, 60)
        w = [base.astype(np.complex64) * np.float32(2.0 ** s) for s in SCALES]
        return SyncCase(name, w, None, 200, truth=[(5, 100)] * len(SCALES), snr=12.0)
    if name == "zero":
        return SyncCase(name, np.zeros((3, 2552), np.complex64), [0.0, 0.1, 0.0], 200, signal=False)
    if name == "zero_m0":
        return SyncCase(name, np.zeros((1, 2552), np.complex64), None, 0, signal=False)
    if name.startswith("batch_"):
        n = int(name.split("_")[1])
        return _batch_case(name, n)
    if name.startswith("fmt_"):
        _, fmt, stride = name.split("_")
        ks = [0, 17, -150]
        ts = [-504, 0, 200]
        w = [prs_window(k + 0.2, t, 12.0, 70 + i) for i, (k, t) in enumerate(zip(ks, ts))]
        fs = [0.0, 0.2 / 2048, -0.5]
        w[2] = prs_window(-150.2, 200, 12.0, 72, correction=-0.5)
        return SyncCase(name, w, fs, 200, truth=[(0, -504), (17, 0), (-150, 200)], fmt=fmt, stride=int(stride), snr=12.0)
    raise KeyError(name)


SCALES = [-40, -21, -1, 0, 1, 17, 40]


@functools.lru_cache(maxsize=None)
def _batch_windows(n):
    """n distinct windows: offsets and noise differ per window."""
    x = _frame(0)
    i = np.arange(n)
    ks = (i * 7) % 61 - 30
    ts = (i * 53) % 1001 - 500
    rng = np.random.default_rng(80)
    idx = (NULL - ts)[:, None] + np.arange(2552)[None, :]
    seg = x[idx].astype(np.complex128)
    seg *= np.exp(2j * np.pi * ((ks + 0.2) / 2048)[:, None] * idx)
    seg += np.sqrt(0.5 * 10 ** -1.2) * (rng.standard_normal(seg.shape) + 1j * rng.standard_normal(seg.shape))
    return seg.astype(np.complex64), list(zip(ks.tolist(), ts.tolist()))


def _batch_case(name, n):
    w, truth = _batch_windows(4097)
    return SyncCase(name, w[:n], None, 64, truth=truth[:n], snr=12.0, batch_D=True)


SYNC_NAMES = (["coarse_0", "coarse_1", "coarse_200", "coarse_1023", "fraction", "time", "nco_wrap", "noise", "scaled",
               "zero", "zero_m0", "batch_1", "batch_300", "batch_4096", "batch_4097"] +
              ["fmt_%s_%d" % (f, s) for f in ("cs16", "cs8", "cu8") for s in (2552, 2553)])


def check_sync_case(case, got):
    """-> (cases, unambiguous, largest error / budget)."""
    n_unamb, worst = 0, 0.0
    for i, s in enumerate(case.refs):
        g = got[i]
        label = "%s[%d]" % (case.name, i)
        worst = max(worst, SR.check_sync(s, int(g["coarse_carriers"]), int(g["time_offset"]), float(g["peak_to_mean"]),
                                         float(g["coarse_peak_to_mean"]), label))
        n_unamb += s.unambiguous
        if case.truth is not None and case.truth[i][0] is not None:
            assert s.unambiguous, "%s: a signal case at >= 8 dB is ambiguous" % label
        if case.truth is not None and case.truth[i][0] is None:
            assert abs(int(g["coarse_carriers"])) <= case.max_coarse
    if case.signal:
        assert n_unamb >= sum(t[0] is not None for t in case.truth)
    if case.name.startswith("zero"):
        assert (got["coarse_carriers"] == 0).all() and (got["time_offset"] == 0).all()
        assert (got["peak_to_mean"] == 0).all() and (got["coarse_peak_to_mean"] == 0).all()
        assert not (got["peak_to_mean"] >= np.float32(1e-30)).any()
    if case.name == "scaled":
        assert (got[1:] == got[:1]).all(), "results differ bit for bit between 2^k scalings: %s" % got
    print("STATS sync %-16s cases %5d unambiguous %5d worst %.3f of budget" % (case.name, len(case.refs), n_unamb, worst))
    return len(case.refs), n_unamb, worst


def run_sync_oracle(case):
    from oracle import oracle as O
    out = np.zeros(len(case.refs), SYNC_DTYPE)
    for i, v in enumerate(case.values):
        f = 0.0 if case.f is None else float(case.f[i])
        out[i] = O.sync_prs(v.astype(np.complex64), f, case.max_coarse)
    return out


# --------------------------------------------------------------------------------------------------- acquisition cases
class AcqCase:
    """Streams [n][n_samples] (values complex), cfg kwargs, max_frames; refs built lazily per candidate."""

    def __init__(self, name, streams, max_frames=16, fmt="cf32", stride_pad=0, signal=True, **cfg):
        self.name, self.fmt, self.max_frames, self.stride_pad = name, fmt, max_frames, stride_pad
        self.cfg = dict(thr_null_start=0.35, thr_null_end=0.75, min_null_blocks=30, max_coarse_carriers=200,
                        min_peak_to_mean=30.0, timing_margin=64, impulse_peak_distance_probability=0.15,
                        first_path_rel=0.25, level_chunk_blocks=256)
        self.cfg.update(cfg)
        s = np.asarray(streams)
        if fmt == "cf32":
            self.q = s.astype(np.complex64)
            self.values = self.q.astype(np.complex128)
        else:
            self.q, self.values = quantise(s, fmt)
        self.signal = signal
        c = self.cfg
        self.ns = [SR.NullSearch(v, c["thr_null_start"], c["thr_null_end"], c["min_null_blocks"], c["level_chunk_blocks"],
                                 max_frames) for v in self.values]
        self._acq = {}

    def acquired(self, st, cand):
        key = (st, cand)
        if key not in self._acq:
            c = self.cfg
            self._acq[key] = SR.Acquired(self.values[st], cand, c["max_coarse_carriers"], c["min_peak_to_mean"],
                                         c["timing_margin"], c["impulse_peak_distance_probability"], c["first_path_rel"])
        return self._acq[key]


def capture(seed, n_frames, cut, length, snr=15.0, cfo=3.3, paths=None, gain=None):
    e = synth.Ensemble(seed=seed, n_frames=n_frames)
    iq = np.tile(e.iq().ravel(), 2)
    x = iq[cut:cut + length]
    rng = np.random.default_rng(seed)
    g = None if gain is None else gain(np.arange(length))
    return synth.channel(x, snr_db=snr, cfo=cfo / 2048.0, rng=rng, paths=paths, gain=g)


def prs_starts(cut, length, n_frames):
    """True PRS prefix starts inside a capture made by capture()."""
    return [k * FRAME + NULL - cut for k in range(2 * n_frames) if 0 <= k * FRAME + NULL - cut < length]


def fake_dips(x, dips):
    """Attenuate [64 b, 64 (b + L)) for every (b, L) by 40 dB."""
    y = x.copy()
    for b, L in dips:
        y[64 * b:64 * (b + L)] *= np.float32(0.01)
    return y


@functools.lru_cache(maxsize=None)
def acq_case(name):
    if name == "unaligned_lengths":
        # lengths that are not a multiple of 64; one capture begins inside a null symbol
        a = capture(1, 3, 70001, 3 * FRAME + 4133, cfo=-7.3)
        b = capture(1, 3, 1300, 3 * FRAME + 4133, cfo=-7.3)
        return AcqCase(name, [a, b])
    if name == "cut_off":
        # the last frame ends 1000 samples early, inside the 512 slack, and 600 samples after it
        ln = [2 * FRAME + NULL + SYMS - 1000, 2 * FRAME + NULL + SYMS + 300, 2 * FRAME + NULL + SYMS + 600]
        return [AcqCase(name + "_%d" % i, [capture(2, 3, 0, L, cfo=2.2)]) for i, L in enumerate(ln)]
    if name == "dip_lengths":
        x = capture(3, 5, 0, 5 * FRAME + 8000, cfo=1.1)
        return AcqCase(name, [fake_dips(x, [(3072 * k + 700, L) for k, L in enumerate([29, 30, 83, 84])])])
    if name == "segment_boundary":
        base = capture(4, 8, 0, 7 * FRAME + 3000, cfo=-2.6)
        streams = [fake_dips(base, [(16384 - o, 40)]) for o in (0, 1, 20, 40)]
        return AcqCase(name, streams, stride_pad=4099)
    if name.startswith("level_chunk_"):
        ch = int(name.split("_")[2])
        n = 5 * FRAME + 777
        x = capture(5, 6, 50000, n, cfo=4.4) * np.where(np.arange(n) < n // 2, 1.0, 0.15).astype(np.float32)
        return AcqCase(name, [x], level_chunk_blocks=ch)
    if name == "max_frames":
        return AcqCase(name, [capture(6, 6, 9000, 6 * FRAME, cfo=0.4)], max_frames=3)
    if name == "streams":
        xs = [capture(7 + i, 3, 5000 * i + 17, 3 * FRAME + 2000, cfo=c) for i, c in enumerate([-20.4, 0.3, 150.1])]
        return AcqCase(name, xs, stride_pad=1024 + 6)
    if name == "half_carrier":
        xs = [capture(8, 3, 30000, 3 * FRAME, snr=s, cfo=7.5) for s in (None, 15.0)]
        return AcqCase(name, xs)
    if name == "cs8":
        xs = [capture(9, 3, 40001, 3 * FRAME + 100, cfo=-11.3, snr=14.0)]
        return AcqCase(name, xs, fmt="cs8")
    if name.startswith("paths_"):
        spec = PATH_CASES[name[6:]]
        xs = [capture(10, 3, 60000, 3 * FRAME, snr=25.0, cfo=-1.2, paths=spec["paths"])]
        return AcqCase(name, xs, **spec["cfg"])
    raise KeyError(name)


# two-path channels (relative amplitudes; synth normalises the total), rel = first_path_rel
PATH_CASES = {
    "early_above_rel": dict(paths=[(0, np.sqrt(0.5)), (200, 1.0)], cfg={}),              # 0.5 = rel x 2 (+3 dB)
    "early_below_rel": dict(paths=[(0, np.sqrt(0.125)), (200, 1.0)], cfg={}),            # rel / 2 (-3 dB)
    "delay_1": dict(paths=[(0, 0.7), (1, 1.0)], cfg={}),
    "delay_504": dict(paths=[(0, 0.7), (504, 1.0)], cfg={}),
    "delay_505": dict(paths=[(0, 0.7), (505, 1.0)], cfg={}),
    "p0": dict(paths=[(0, 1.0), (300, 1.1)], cfg=dict(impulse_peak_distance_probability=0.0, first_path_rel=0.0)),
    "p015": dict(paths=[(0, 1.0), (300, 1.1)], cfg=dict(impulse_peak_distance_probability=0.15, first_path_rel=0.0)),
    "p1": dict(paths=[(0, 1.0), (300, 1.1)], cfg=dict(impulse_peak_distance_probability=1.0, first_path_rel=0.0)),
    "floor_decides": dict(paths=[(0, 0.055), (150, 1.0)], cfg=dict(first_path_rel=0.001)),
    "two_early": dict(paths=[(0, 0.6), (100, 0.7), (250, 1.0)], cfg={}),
}

ACQ_NAMES = (["unaligned_lengths", "cut_off", "dip_lengths", "segment_boundary", "max_frames", "streams", "half_carrier",
              "cs8"] + ["level_chunk_%d" % c for c in (0, 64, 256, 16384)] + ["paths_" + k for k in PATH_CASES])


def _cases(name):
    c = acq_case(name)
    return c if isinstance(c, list) else [c]


def check_acq_case(case, frames, counts):
    """frames [n_streams][max_frames] records, counts [n_streams] -> (frames checked, unambiguous, worst)."""
    n, n_unamb, n_branch, worst = 0, 0, 0, 0.0
    for st, ns in enumerate(case.ns):
        cnt = int(counts[st])
        alts = [a for a in ns.alternatives if len(a) == cnt]
        assert alts, "%s stream %d: %d frames, the reference allows %s" % (case.name, st, cnt,
                                                                          sorted(len(a) for a in ns.alternatives))
        errs = []
        for alt in alts:
            try:
                w = 0.0
                for j, cand in enumerate(alt):
                    w = max(w, SR.check_acquired(case.acquired(st, cand), frames[st][j],
                                                 "%s s%d f%d cand %d" % (case.name, st, j, cand)))
                break
            except AssertionError as e:
                errs.append(str(e))
        else:
            raise AssertionError("; ".join(errs))
        worst = max(worst, w)
        for j in range(cnt, case.max_frames):
            assert int(frames[st][j]["start"]) == -1 and int(frames[st][j]["flags"]) == 0
        for j, cand in enumerate(alt):
            a = case.acquired(st, cand)
            n += 1
            u = a.unambiguous and ns.unambiguous
            n_unamb += u
            if case.signal and (frames[st][j]["flags"] & 1) and a.sync.ptm > 1000 and len(a.branches) == 1:
                assert u, "%s s%d f%d: a locked frame at high SNR is ambiguous" % (case.name, st, j)
            n_branch += len(a.branches) == 2
    print("STATS acq  %-24s frames %4d unambiguous %4d half-carrier branch %d worst %.3f of budget" %
          (case.name, n, n_unamb, n_branch, worst))
    return n, n_unamb, worst


def run_acq_oracle(case):
    from oracle import oracle as O
    import dabgpu
    c = case.cfg
    S = len(case.values)
    frames = np.zeros((S, case.max_frames), dabgpu.ACQUIRED_FRAME_DTYPE)
    frames["start"] = -1
    counts = np.zeros(S, np.int32)
    for st, v in enumerate(case.values):
        x = v.astype(np.complex64)
        cands = O.null_search(x, c["thr_null_start"], c["thr_null_end"], c["min_null_blocks"], case.max_frames,
                              c["level_chunk_blocks"])
        counts[st] = len(cands)
        for j, cand in enumerate(cands):
            r = O.acquire_candidate(x, cand, c["max_coarse_carriers"], c["min_peak_to_mean"], c["timing_margin"],
                                    c["impulse_peak_distance_probability"], c["first_path_rel"])
            for f in dabgpu.ACQUIRED_FRAME_DTYPE.names:
                frames[st, j][f] = getattr(r, f)
    return frames, counts


# --------------------------------------------------------------------------------------------------- CPU
def test_reference_recovers_transmitted_offsets():
    n_checked = 0
    for name in ["coarse_200", "coarse_1023", "fraction", "time", "nco_wrap", "batch_300"]:
        case = sync_case(name)
        for s, (k, t) in zip(case.refs, case.truth):
            if k is None:
                continue
            assert (s.k, s.t) == (k, t), (name, s.k, s.t, k, t)
            assert s.ptm > 100 and s.cptm > 10
            n_checked += 1
    assert n_checked > 300
    # whole-frame starts of an acquisition: PRS prefix = start + margin
    case = _cases("streams")[0]
    for st, ns in enumerate(case.ns):
        truth = [p for p in prs_starts(5000 * st + 17, case.values.shape[1], 3) if p + SYMS + 512 <= case.values.shape[1]]
        assert len(ns.cands) == len(truth)
        for cand, p in zip(ns.cands, truth):
            a = case.acquired(st, cand)
            assert a.start() + 64 == p
            assert a.sync.k == int(np.rint([-20.4, 0.3, 150.1][st]))


def test_direct_sum_equals_fft_correlation():
    for name in ["coarse_1023", "time", "noise"]:
        case = sync_case(name)
        for s in case.refs:
            D = SR.coarse_fft(s.Q, case.max_coarse)
            assert np.abs(D - s.D).max() <= 1e-12 * np.abs(s.D).max()


def test_zero_window_definition():
    s = SR.Sync(np.zeros(2552), 0.0, 200, first_path_rel=0.25)
    assert (s.k, s.t, s.ptm, s.cptm) == (0, 0, 0.0, 0.0)


@pytest.mark.parametrize("name", SYNC_NAMES)
def test_oracle_sync_within_reference_bands(built, name):
    case = sync_case(name)
    check_sync_case(case, run_sync_oracle(case))


@pytest.mark.parametrize("name", ACQ_NAMES)
def test_oracle_acquire_within_reference_bands(built, name):
    for case in _cases(name):
        check_acq_case(case, *run_acq_oracle(case))


def test_acquire_cases_exercise_their_edges():
    """The cases do what they are named for, per the reference."""
    c = acq_case("dip_lengths")
    found = [(cand // 64 + 1) for cand in c.ns[0].cands]
    ends = {3072 * k + 700 + L: L for k, L in enumerate([29, 30, 83, 84])}
    assert sorted(ends[e] for e in found if e in ends) == [30, 83]
    cut = _cases("cut_off")
    assert [len(c.ns[0].cands) for c in cut] == [2, 2, 3]
    # a level step: against the capture's mean the quiet half is one long dip; the local level finds its frames
    n_lc = {c: len(acq_case("level_chunk_%d" % c).ns[0].cands) for c in (0, 64, 256, 16384)}
    assert n_lc[0] < n_lc[64] and n_lc[0] < n_lc[256]
    seg = acq_case("segment_boundary")
    assert all(any(abs(cand - (16384 - o + 40) * 64 + 48) == 0 for cand in ns.cands) for o, ns in zip((0, 1, 20, 40), seg.ns))
    mf = acq_case("max_frames")
    assert len(mf.ns[0].cands) == 3 and len(SR.NullSearch(mf.values[0], max_out=64).cands) > 3
    hc = acq_case("half_carrier")
    assert len(hc.acquired(0, hc.ns[0].cands[0]).branches) == 2          # noise-free: the angle is pi within its band
    # the tap each two-path channel is aligned to, relative to the first path (the true PRS prefix)
    want = {"early_above_rel": 0, "early_below_rel": 200, "delay_1": 0, "delay_504": 0, "delay_505": 505, "p1": 300, "floor_decides": 150, "two_early": 0}
    for k, d in want.items():
        c = acq_case("paths_" + k)
        truth = prs_starts(60000, c.values.shape[1], 3)
        for cand in c.ns[0].cands:
            a = c.acquired(0, cand)
            p = min(truth, key=lambda q: abs(q - cand))
            got = cand + a.sync.t - p
            if k == "floor_decides":                 # the strongest path's own first significant tap: its sidelobes
                assert d - 8 <= got <= d, (k, got)   # reach 16 x mean, the 0.3 % path at 0 does not
            else:
                assert got == d, (k, got)


# --------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def run_sync_gpu(ctx, case, dev_call=False):
    import dabgpu
    if case.fmt == "cf32" and not dev_call:
        rows = np.zeros((len(case.q), case.stride), np.complex64)
        rows[:, :2552] = case.q
        return ctx.sync_prs(rows, case.f, case.max_coarse)
    torch, dev = _torch()
    n = len(case.q)
    if case.fmt == "cf32":
        flat = np.zeros((n, case.stride), np.complex64)
        flat[:, :2552] = case.q
        buf = torch.from_numpy(flat.view(np.float32).reshape(-1)).to(dev)
    else:
        dt = {"cs16": np.int16, "cs8": np.int8, "cu8": np.uint8}[case.fmt]
        flat = np.zeros((n, case.stride, 2), dt)
        flat[:, :2552] = case.q
        buf = torch.from_numpy(flat.reshape(-1)).to(dev)
        ctx.set_iq_format({"cs16": dabgpu.IQ_CS16, "cs8": dabgpu.IQ_CS8, "cu8": dabgpu.IQ_CU8}[case.fmt])
    try:
        fo = None if case.f is None else torch.from_numpy(case.f).to(dev)
        out = torch.zeros(n * 4, dtype=torch.int32, device=dev)
        ctx.sync_prs_dev(buf.data_ptr(), case.stride, n, None if fo is None else fo.data_ptr(), case.max_coarse,
                         out.data_ptr())
        ctx.sync()
        return out.cpu().numpy().view(SYNC_DTYPE)
    finally:
        ctx.set_iq_format(dabgpu.IQ_CF32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SYNC_NAMES)
def test_gpu_sync_against_reference(gctx, name):
    case = sync_case(name)
    got = run_sync_gpu(gctx, case)
    check_sync_case(case, got)
    if case.fmt == "cf32" and name in ("coarse_200", "time", "zero", "batch_300"):
        dev = run_sync_gpu(gctx, case, dev_call=True)
        assert (dev == got).all()


@pytest.mark.gpu
def test_gpu_sync_rejects_odd_cf32_stride(gctx):
    import dabgpu
    torch, dev = _torch()
    buf = torch.zeros(2 * 2553 * 2, dtype=torch.float32, device=dev)
    out = torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(dabgpu.DabGpuError):
        gctx.sync_prs_dev(buf.data_ptr(), 2553, 2, None, 200, out.data_ptr())


def run_acq_gpu(ctx, case):
    import dabgpu
    cfg = dabgpu.acquire_cfg(**case.cfg)
    S, n = case.values.shape
    if case.fmt == "cf32" and case.stride_pad == 0:
        return ctx.acquire(case.q, case.max_frames, cfg)
    torch, dev = _torch()
    stride = n + case.stride_pad
    if case.fmt == "cf32":
        flat = np.zeros((S, stride), np.complex64)
        flat[:, :n] = case.q
        buf = torch.from_numpy(flat.view(np.float32).reshape(-1)).to(dev)
    else:
        dt = {"cs16": np.int16, "cs8": np.int8, "cu8": np.uint8}[case.fmt]
        flat = np.zeros((S, stride, 2), dt)
        flat[:, :n] = case.q
        buf = torch.from_numpy(flat.reshape(-1)).to(dev)
        ctx.set_iq_format({"cs16": dabgpu.IQ_CS16, "cs8": dabgpu.IQ_CS8, "cu8": dabgpu.IQ_CU8}[case.fmt])
    try:
        out = torch.zeros(S * case.max_frames * 32, dtype=torch.uint8, device=dev)
        counts = torch.zeros(S, dtype=torch.int32, device=dev)
        ctx.acquire_dev(buf.data_ptr(), stride, S, n, case.max_frames, out.data_ptr(), counts.data_ptr(), cfg)
        ctx.sync()
        fr = out.cpu().numpy().view(dabgpu.ACQUIRED_FRAME_DTYPE).reshape(S, case.max_frames)
        return fr, counts.cpu().numpy()
    finally:
        ctx.set_iq_format(dabgpu.IQ_CF32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ACQ_NAMES)
def test_gpu_acquire_against_reference(gctx, name):
    for case in _cases(name):
        check_acq_case(case, *run_acq_gpu(gctx, case))
