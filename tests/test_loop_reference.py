"""The frequency and timing loops -- stream_update_kernel, track_update_kernel, track_start_kernel and the MODE_TRACK
branch of prs_sync_kernel -- against the float64 from-definition reference tests/loop_reference.py, at the sizes where
the kernels change path: 1, 2, 13, 14 (14 x 76 > 1024: a thread's second entry), 107, 108 (108 x 76 > 8192: two live
batches) and 216 frames (the outer loop's second trip); track_start at 63, 64, 65 and 130 records (its lane loop).

Bars (derived in the reference's docstring): every float of the state within its budget, every integer exact, discrete
outcomes (level_lost, quality gate, branch, wrap) exact unless the reference value lies within its budget of the
threshold -- only the cases named edge_* may, and they assert that they do.
CPU part: known answers; the float32 oracle under the same bars on the inputs of every GPU case (synthetic arrays of the
same shapes, lock patterns and prior states); the sensitivity of the bars (a frame's 76 entries dropped or counted
twice, a locked slot's residual dropped, move the reference by more than 4 budgets); the ambiguity cap; no budget above
the bar test_tracking.check_state uses.  GPU part: teacher-forced -- the reference is fed the state before each call and
the call's own device outputs (correlations, frame records; in decision-directed mode the sums of
dabgpu_ofdm_demod_frames_dd_dev on the same samples with the pre-call offset) and the state after is held to it."""
import functools
import types

import numpy as np
import pytest

import loop_reference as LR
from dabgpu import synth

L = LR.L_FRAME
NULL = synth.NB_NULL
SYMS = LR.FRAME_LEN
MARGIN = 64
SIZES = (1, 2, 13, 14, 107, 108, 216)
NOB = LR.DD_NO_BRANCH
REPORT = {}


def note(group, frac, unambiguous, total):
    r = REPORT.setdefault(group, {"worst": {}, "unambiguous": 0, "cases": 0})
    for k, v in frac.items():
        r["worst"][k] = max(r["worst"].get(k, 0.0), v)
    r["unambiguous"] += unambiguous
    r["cases"] += total


def show(group):
    r = REPORT.get(group)
    if r:
        print("\n%s: largest error / budget %s; %d of %d cases unambiguous" %
              (group, " ".join("%s %.3f" % kv for kv in sorted(r["worst"].items())), r["unambiguous"], r["cases"]))


def spread(rng, n):
    """Per-frame residual offsets in carriers: spread over +-0.05 in pairs +m, -m (shuffled), none within 0.01 of zero.  The
    call's mean (and the angle of its fourth-power sum) then stays near zero, no frame sits on it, and so every frame's
    presence shows in the estimate -- what the sensitivity test asserts."""
    m = rng.uniform(0.01, 0.05, (n + 1) // 2)
    d = np.concatenate([m, -m])[:n]
    rng.shuffle(d)
    return d


# ------------------------------------------------------------------------------------------------------ stream cases
def stream_case(name, F, dd):
    """Streams of one stream call: per stream the carrier offset c (carriers), the level, the per-frame residuals and the
    prior state written before the call."""
    rng = np.random.default_rng(1000 + F + 7 * dd)
    S = 3 if F <= 14 else 2
    streams = []
    for s in range(S):
        c = (0.21, -0.33, 0.08)[s]
        amp = (1.0, 0.25, 3.0)[s]
        pre = dict(fine_freq_offset=float(np.float32(-c / 2048.0)))
        if s == 1:                                                # a running average near the level, a loop that was locked
            pre.update(signal_average=1.1 * amp, total_frames_read=10, dd_branch=0, dd_pending=NOB, total_frames_desync=1)
        if s == 2:                                                # the level is lost against the average so far
            pre.update(signal_average=5.0 * amp, total_frames_read=7, dd_branch=0, dd_pending=NOB, loop_gated=2)
        streams.append(dict(c=c, amp=amp, delta=spread(rng, F), pre=pre))
    return dict(name=name, F=F, dd=dd, streams=streams, stride=SYMS, seed=int(rng.integers(1 << 30)), gate=2.5)


def stream_wrap_case(dd):
    """Fine offsets 0.01 carriers inside +-half a carrier, residuals that push them over: both wrap."""
    rng = np.random.default_rng(77 + dd)
    streams = []
    for sign in (1.0, -1.0):
        fine = float(np.float32(sign * 0.49 / 2048.0))
        streams.append(dict(c=-sign * 0.49, amp=1.0, delta=-sign * rng.uniform(0.035, 0.045, 2),
                            pre=dict(fine_freq_offset=fine, signal_average=1.1, total_frames_read=4, dd_branch=0, dd_pending=NOB)))
    return dict(name="wrap", F=2, dd=dd, streams=streams, stride=SYMS + 38, seed=5 + dd, gate=2.5)


@functools.lru_cache(maxsize=None)
def stream_cases():
    out = []
    for dd in (0, 1):
        out += [stream_case("F%d" % F, F, dd) for F in SIZES]
        out.append(stream_wrap_case(dd))
    return out


def synth_rows(rng, resid, amp, dd):
    """Loop input of frames with the given residual offsets (carriers) as a front end would hand it over: cyclic-prefix
    correlations, or fourth-power sums behind the PRS's correlation."""
    resid = np.asarray(resid, np.float64)
    F = resid.size
    th = 2 * np.pi * resid[:, None] + 0.02 * rng.standard_normal((F, 76))
    rows = 500.0 * amp * amp * (1 + 0.1 * rng.standard_normal((F, 76))) * np.exp(1j * th)
    if dd:
        ph4 = 4 * 2 * np.pi * 2552 * (resid / 2048.0)
        rows[:, 1:] = -150.0 * np.exp(1j * (ph4[:, None] + 0.05 * rng.standard_normal((F, 75)))) + \
            3.0 * (rng.standard_normal((F, 75)) + 1j * rng.standard_normal((F, 75)))
    return rows.astype(np.complex64)


def synth_level(rng, amp):
    x = amp * np.sqrt(0.5) * (rng.standard_normal(4096) + 1j * rng.standard_normal(4096))
    return x.astype(np.complex64)


def stream_synthetic(case):
    """-> per stream (state, rows, last frame's samples) from synthetic arrays."""
    rng = np.random.default_rng(case["seed"])
    out = []
    for st in case["streams"]:
        state = q32(LR.fresh_state(**st["pre"]))
        resid = st["delta"] + st["c"] + float(np.float32(state["fine_freq_offset"])) * 2048.0
        out.append((state, synth_rows(rng, resid, st["amp"], case["dd"]), synth_level(rng, st["amp"])))
    return out


def q32(state):
    """The state as the device holds it: every float but next_frame_start a float32."""
    return {k: (float(np.float32(v)) if isinstance(v, float) and k != "next_frame_start" else v) for k, v in state.items()}


def f32_state(state):
    d = dict(state)
    for k in ("fine_freq_offset", "coarse_freq_offset", "signal_average", "last_fine_error", "drift", "last_peak_to_mean"):
        d[k] = np.float32(d[k])
    return d


def check_budgets(outcomes, what):
    for o in outcomes:
        assert not LR.budgets_within_bars(o), (what, LR.budgets_within_bars(o))


# ------------------------------------------------------------------------------------------------------ tracked cases
def lock_plan(C, s, rng):
    """Unlocked slots: the first, the last and slots 13, 107, 108 beside random ones -- no period in them."""
    if C == 1:
        return {0} if s == 1 else set()
    if C == 2:
        return {0} if s == 1 else {1}
    bad = {0, C - 1} | {i for i in (13, 107, 108) if i < C}
    bad |= {int(i) for i in rng.choice(C, max(1, C // 10), replace=False)}
    if len(bad) > C - 3:
        bad = set(sorted(bad)[:C - 3])
    return bad


def tracked_stream(rng, C, ppm, c, amp, unlocked, pre=None, j0=0, next_err=0.37, drift_err=0.02):
    """One stream of a tracked call: frames on a period of 196608 (1 + ppm e-6) with +-2 samples of jitter, a state whose
    prediction is 0.37 samples and 0.02 samples per frame off.  The jitter is drawn again until no locked start lies on
    the line through the others (integer jitter can put one there exactly, and a point on the line says nothing about
    whether it was counted)."""
    period = L * (1.0 + ppm * 1e-6)
    P0 = 3000
    drift = float(np.float32(ppm * 1e-6 * L + drift_err))
    state = dict(fine_freq_offset=float(np.float32(-c / 2048.0)), tracking=1, drift=drift, signal_average=1.1 * amp,
                 next_frame_start=P0 + next_err - j0 * (L + drift), total_frames_read=20, dd_branch=0, dd_pending=NOB)
    state.update(pre or {})
    locked = np.array([i for i in range(C) if i not in unlocked], np.int64)
    while True:
        pos = P0 + np.rint(np.arange(C + 1) * period).astype(np.int64)
        pos[:C] += rng.integers(-2, 3, C)
        if locked.size < 3:
            break
        r = pos[locked] - (state["next_frame_start"] + (j0 + locked) * (L + drift))
        fit = np.polyfit(locked.astype(np.float64), r, 1)
        if np.abs(r - np.polyval(fit, locked)).min() > 0.01:
            break
    return dict(C=C, ppm=ppm, c=c, amp=amp, pos=pos, unlocked=set(unlocked), delta=spread(rng, C), state=state, j0=j0)


def tracked_case(name, streams, dd=0, gate=2.5, seed=0):
    C = streams[0]["C"]
    n_samples = int(max(int(st["pos"][C - 1]) for st in streams) + SYMS + LR.FIT_SLACK + 1000)
    assert all(st["C"] == C and int(st["pos"][C]) + SYMS + LR.FIT_SLACK > n_samples + 8 for st in streams)
    return dict(name=name, C=C, MF=C + 2, n_samples=n_samples, advance=C * L, streams=streams, dd=dd, gate=gate, seed=seed)


@functools.lru_cache(maxsize=None)
def tracked_size_cases():
    out = []
    for C in SIZES:
        rng = np.random.default_rng(2000 + C)
        S = 1 if C >= 107 else 2
        sts = []
        for s in range(S):
            ppm = float(rng.uniform(60, 150)) * (1 if (s + C) % 2 else -1)
            sts.append(tracked_stream(rng, C, ppm, (0.17, -0.29)[s], (1.0, 0.4)[s], lock_plan(C, s, rng)))
        out.append(tracked_case("C%d" % C, sts, seed=C))
    return out


@functools.lru_cache(maxsize=None)
def tracked_edge_cases():
    rng = np.random.default_rng(31)
    five, one = [], []

    def add(lst, C, name, unlocked, **kw):
        ppm = float(rng.uniform(60, 150)) * rng.choice([-1, 1])
        st = tracked_stream(rng, C, ppm, float(rng.uniform(-0.3, 0.3)), 1.0, unlocked, **kw)
        st["name"] = name
        lst.append(st)

    add(five, 5, "none_locked", {0, 1, 2, 3, 4})
    add(five, 5, "one_of_several", {0, 1, 3, 4})
    add(five, 5, "two_locked", {0, 2, 4})
    add(five, 5, "three_locked", {1, 3})
    add(five, 5, "four_locked", {2})
    add(five, 5, "five_locked", set())
    add(five, 5, "skipped_samples", {1}, j0=2)
    add(five, 5, "level_lost_several", {0}, pre=dict(signal_average=5.0))
    add(five, 5, "no_average_yet", {4}, pre=dict(signal_average=0.0))
    for sign, nm in ((1.0, "wrap_plus"), (-1.0, "wrap_minus")):
        add(five, 5, nm, {2})
        five[-1]["c"] = -sign * 0.49
        five[-1]["state"]["fine_freq_offset"] = float(np.float32(sign * 0.49 / 2048.0))
        five[-1]["delta"] = -sign * rng.uniform(0.035, 0.045, 5)
    add(one, 1, "one_of_one", set())
    add(one, 1, "level_lost_single", set(), pre=dict(signal_average=5.0))
    add(one, 1, "none_of_one", {0})
    dd = []
    add(dd, 2, "dd_after_start", set(), pre=dict(dd_branch=NOB, dd_pending=NOB, total_frames_read=2))
    add(dd, 2, "dd_locked", set())
    for nm, pend in (("dd_branch_held", NOB), ("dd_branch_believed", 1)):
        add(dd, 2, nm, set(), pre=dict(dd_pending=pend))
        dd[-1]["delta"] = np.array([0.19, 0.21])                 # one branch (0.2 carriers) away
    add(dd, 2, "dd_level_lost", {0}, pre=dict(signal_average=5.0, dd_pending=1, loop_gated=3))
    return [tracked_case("edges5", five, seed=11), tracked_case("edges1", one, seed=12),
            tracked_case("edges_dd", dd, dd=1, seed=13), tracked_case("edges_dd_gated", dd, dd=1, gate=500.0, seed=14)]


def tracked_synthetic(case):
    """-> per stream (state, frame records, rows, level samples) from synthetic arrays."""
    rng = np.random.default_rng(case["seed"] + 99)
    out = []
    for st in case["streams"]:
        C = case["C"]
        state = q32(LR.fresh_state(**st["state"]))
        fr = np.zeros(case["MF"], FRAME_DTYPE)
        fr["start"], fr["flags"] = -1, 0
        for i in range(C):
            ok = i not in st["unlocked"]
            fr[i]["start"], fr[i]["flags"] = int(st["pos"][i]), 3 if ok else 2
            fr[i]["peak_to_mean"] = np.float32(rng.uniform(300, 900) if ok else rng.uniform(5, 20))
        resid = st["delta"] + st["c"] + float(np.float32(state["fine_freq_offset"])) * 2048.0
        rows = np.zeros((case["MF"], 76), np.complex64)
        rows[:C] = synth_rows(rng, resid, st["amp"], case["dd"])
        out.append((state, fr, rows, synth_level(rng, st["amp"])))
    return out


FRAME_DTYPE = np.dtype([("start", np.int64), ("freq_offset", np.float32), ("coarse_carriers", np.int32),
                        ("fine_offset", np.float32), ("peak_to_mean", np.float32), ("coarse_peak_to_mean", np.float32),
                        ("flags", np.int32)])


def tracked_reference(case, state, fr, rows, level, ds_input=0.0):
    return LR.track_update(state, fr, rows, level, case["n_samples"], case["MF"], case["advance"], dd=bool(case["dd"]),
                           dd_gate=case["gate"], ds_input=ds_input)


# ------------------------------------------------------------------------------------------------------ start cases
START_COUNTS = (1, 3, 4, 5, 63, 64, 65, 130)
START_MF = 130


@functools.lru_cache(maxsize=None)
def start_streams():
    """One launch: per stream (name, records [START_MF], counts[s], prior state)."""
    rng = np.random.default_rng(4242)
    out = []

    def records(n, ppm, unlocked=()):
        fr = np.zeros(START_MF, FRAME_DTYPE)
        fr["start"] = -1
        j = np.arange(n)
        j = j + (j >= 2) + 2 * (j >= max(3, n // 2))             # one missed frame, then two more
        start = 5000 + np.rint(j * L * (1 + ppm * 1e-6)).astype(np.int64) + rng.integers(-2, 3, n)
        fr["start"][:n] = start
        fr["flags"][:n] = 3
        for i in unlocked:
            fr["flags"][i] = 2
        fr["fine_offset"][:n] = rng.uniform(-2.4e-4, 2.4e-4, n).astype(np.float32)
        fr["coarse_carriers"][:n] = rng.integers(-30, 30, n)
        fr["peak_to_mean"][:n] = rng.uniform(100, 900, n).astype(np.float32)
        return fr

    def prior(k):
        return q32(LR.fresh_state(tracking=k % 2, total_frames_read=3 * k, dd_branch=0, dd_pending=1, drift=0.5, next_frame_start=123.0,
                              fine_freq_offset=1e-5, last_time_offset=3))

    for k, n in enumerate(START_COUNTS):
        out.append(("n%d" % n, records(n, float(rng.uniform(-150, 150))), n, prior(k)))
    out.append(("ends_unlocked_5", records(5, 90.0, (0, 4)), 5, prior(1)))
    out.append(("ends_unlocked_4", records(4, -70.0, (0, 3)), 4, prior(0)))
    out.append(("ends_unlocked_65", records(65, 120.0, (0, 64)), 65, prior(0)))
    out.append(("ends_unlocked_130", records(130, -110.0, (0, 1, 128, 129)), 130, prior(1)))
    out.append(("none_locked", records(3, 50.0, (0, 1, 2)), 3, prior(1)))
    out.append(("count_over_max", records(130, 75.0), 140, prior(0)))
    return out


# ======================================================================================================== CPU
def test_reference_known_answers():
    """Correlations built with chosen angles, starts on a chosen line, and the records of a start on a chosen period give
    what the definitions say, by hand."""
    # cyclic-prefix loop: frame f at residual d_f carriers -> err = mean(d) / 2048; level, first-value rule, counters
    d = np.array([0.03, -0.01, 0.05])
    rows = (200.0 * np.exp(2j * np.pi * d))[:, None] * np.ones((1, 76))
    x = np.full(4096, 0.5 - 0.25j)
    st = LR.fresh_state(fine_freq_offset=1e-5)
    (o,) = LR.stream_update(st, rows, x, 0.5)
    assert abs(o["last_fine_error"] - d.mean() / 2048) < 1e-18 and abs(o["fine_freq_offset"] - (1e-5 - 0.5 * d.mean() / 2048)) < 1e-18
    assert o["signal_average"] == 0.75 and o["total_frames_read"] == 3 and o["total_frames_desync"] == 0 and not o["level_lost"]
    # running average; a lost level: one desync, the average stays, several frames still steer; one frame does not
    (o,) = LR.stream_update(LR.fresh_state(signal_average=1.0), rows, x, 0.5, signal_beta=0.5)
    assert abs(o["signal_average"] - 0.875) < 1e-15
    (o,) = LR.stream_update(LR.fresh_state(signal_average=3.0, total_frames_read=5), rows, x, 0.5)
    assert o["level_lost"] and o["steers"] and o["total_frames_desync"] == 1 and o["total_frames_read"] == 7 and o["signal_average"] == 3.0
    (o,) = LR.stream_update(LR.fresh_state(signal_average=3.0, fine_freq_offset=2e-5, dd_branch=4), rows[:1], x, 0.5)
    assert not o["steers"] and o["fine_freq_offset"] == 2e-5 and o["total_frames_read"] == 0 and o["total_frames_desync"] == 1
    assert abs(o["last_fine_error"] - 0.03 / 2048) < 1e-18
    # the wrap: 0.49 carriers, error -0.04 carriers, beta 1 -> 0.53 -> -0.47
    rows_w = (200.0 * np.exp(2j * np.pi * -0.04)) * np.ones((2, 76))
    (o,) = LR.stream_update(LR.fresh_state(fine_freq_offset=0.49 / 2048), rows_w, x, 1.0)
    assert abs(o["fine_freq_offset"] * 2048 + 0.47) < 1e-12 and not o["wrap_edge"]
    # the line: integer positions (drift 0), starts = p_i + 3 + 2 i on slots 0, 2, 3 of 5 -> alpha 3, slope 2
    st = LR.fresh_state(tracking=1, next_frame_start=1000.0, signal_average=0.7)
    fr = np.zeros(7, FRAME_DTYPE)
    n_samples = 1000 + 4 * L + SYMS + 512 + 100
    for i in range(5):
        fr[i]["start"], fr[i]["flags"], fr[i]["peak_to_mean"] = 1000 + i * L + 3 + 2 * i, 3 if i in (0, 2, 3) else 1, 100 + i
    rows5 = 200.0 * np.ones((7, 76), np.complex128)
    outs, count = LR.track_update(st, fr, rows5, x, n_samples, 7, 5 * L - 50, drift_beta=0.5)
    (o,) = outs
    assert count == 5 and abs(o["alpha"] - 3) < 1e-9 and abs(o["slope"] - 2) < 1e-9
    assert abs(o["next_frame_start"] - (1000 + 5 * L + 3 + 10 - (5 * L - 50))) < 1e-9 and abs(o["drift"] - 0.5 * 0.75 * 2) < 1e-9
    assert o["total_frames_read"] == 3 and o["total_frames_desync"] == 2 and o["last_time_offset"] == 9 and o["last_peak_to_mean"] == 103
    # ... the caller skipped two periods: j0 = 2 counts two more lost frames, the slots are the same
    st2 = dict(st, next_frame_start=1000.0 - 2 * L)
    (o2,), count = LR.track_update(st2, fr, rows5, x, n_samples, 7, 5 * L - 50)
    assert count == 5 and o2["total_frames_desync"] == 4 and abs(o2["next_frame_start"] - o["next_frame_start"]) < 1e-9
    # one frame: alone in its call its residual is the drift error (gain beta / 8); among several it says nothing
    fr1 = fr.copy()
    fr1["flags"][[0, 2]] = 1
    (o,), _ = LR.track_update(st, fr1, rows5, x, n_samples, 7, 0)
    assert o["drift"] == 0.0 and abs(o["next_frame_start"] - (1000 + 5 * L + 9)) < 1e-9
    (o,), count = LR.track_update(st, fr[3:], rows5, x, 1000 + SYMS + 512 + 5000, 7, 0)
    assert count == 1 and abs(o["drift"] - 0.5 * 0.125 * (3 * L + 9)) < 1e-6
    # nothing locked: tracking drops, everything counted lost
    fr0 = fr.copy()
    fr0["flags"] = 2
    (o,), _ = LR.track_update(st, fr0, rows5, None, n_samples, 7, 0)
    assert o["tracking"] == 0 and o["total_frames_desync"] == 5 and o["total_frames_read"] == 0 and o["fine_freq_offset"] == 0.0
    # track_start: frame numbers 0, 1, 3, 4, 7 on a period of 196608 + 20 -> drift 20; three records -> 0
    j = np.array([0, 1, 3, 4, 7])
    fs = np.zeros(5, FRAME_DTYPE)
    fs["start"], fs["flags"], fs["fine_offset"], fs["coarse_carriers"], fs["peak_to_mean"] = 777 + j * (L + 20), 3, 1e-5 * (j + 1), -3, 500
    o = LR.track_start(LR.fresh_state(total_frames_read=2), fs, 5, 8, 4 * L)
    assert o["drift"] == 20.0 and o["next_frame_start"] == 777 + 7 * (L + 20) + L + 20 - 4 * L and o["tracking"] == 1
    assert abs(o["fine_freq_offset"] - 4e-5) < 1e-11 and o["coarse_freq_offset"] == 3 / 2048
    assert o["total_frames_read"] == 7 and o["dd_branch"] == NOB and o["dd_pending"] == NOB
    o = LR.track_start(LR.fresh_state(), fs, 3, 8, 0)
    assert o["drift"] == 0.0 and o["next_frame_start"] == 777 + 3 * (L + 20) + L
    o = LR.track_start(LR.fresh_state(tracking=1, drift=0.25), fs, 5, 8, 0, only_lost=True)
    assert o["drift"] == 0.25 and o["tracking"] == 1
    assert LR.track_start(LR.fresh_state(), fs, 5, 8, 0, only_lost=True)["tracking"] == 2
    # prediction: the list ends at the first slot that does not fit
    j0, slots, _ = LR.predict(LR.fresh_state(next_frame_start=-L - 10.25, drift=1.0), 3 * L, 9)
    assert j0 == 2 and slots == [L - 8, 2 * L - 7]


def test_reference_gate_sequence_by_hand():
    """The decision-directed estimate through five calls, walked by hand: the first call believes branch +1; a locked loop
    (branch 0) that sees +1 holds it once, believes it the second time; a weak sum falls back to the PRS prefixes and a held
    level leaves the gate's memory alone."""
    def rows(resid, mag=150.0):
        r = np.zeros((2, 76), np.complex128)
        r[:, 0] = 300.0 * np.exp(2j * np.pi * resid)
        r[:, 1:] = -mag * np.exp(1j * 4 * 2 * np.pi * 2552 * resid / 2048.0)
        return r
    x = np.full(4096, 1.0 + 0j)
    st = LR.fresh_state()
    (o,) = LR.stream_update(st, rows(0.21), x, 0.0, dd=True)                     # first call: everything is believed
    assert (o["dd_branch"], o["dd_pending"], o["loop_gated"]) == (1, NOB, 0) and abs(o["last_fine_error"] * 2048 - 0.21) < 1e-9
    st = {k: o[k] for k in LR.fresh_state()}
    (o,) = LR.stream_update(st, rows(0.03), x, 0.0, dd=True)                     # pulled in: branch 0
    assert (o["dd_branch"], o["dd_pending"], o["loop_gated"]) == (0, NOB, 0)
    st = {k: o[k] for k in LR.fresh_state()}
    (o,) = LR.stream_update(st, rows(0.21), x, 0.0, dd=True)                     # +1 seen once: held
    assert (o["dd_branch"], o["dd_pending"], o["loop_gated"]) == (0, 1, 1)
    assert abs(o["last_fine_error"] * 2048 - (0.21 - 2048.0 / (4 * 2552))) < 1e-9
    st = {k: o[k] for k in LR.fresh_state()}
    lost = dict(st, signal_average=9.0)
    (o1,) = LR.stream_update(lost, rows(0.21)[:1], x, 0.0, dd=True)              # not applied: the memory stays
    assert (o1["dd_branch"], o1["dd_pending"], o1["loop_gated"]) == (0, 1, 1) and not o1["steers"]
    (o,) = LR.stream_update(st, rows(0.21), x, 0.0, dd=True)                     # seen again: believed
    assert (o["dd_branch"], o["dd_pending"], o["loop_gated"]) == (1, NOB, 1) and abs(o["last_fine_error"] * 2048 - 0.21) < 1e-9
    st = {k: o[k] for k in LR.fresh_state()}
    (o,) = LR.stream_update(st, rows(-0.12, mag=0.01), x, 0.0, dd=True)          # |S|^2 = (150 x 0.01)^2 < 2.5^2 x 38400
    assert (o["dd_branch"], o["dd_pending"], o["loop_gated"]) == (-1, NOB, 2) and abs(o["last_fine_error"] * 2048 + 0.12) < 1e-9
    # on the quality threshold both outcomes come back
    S = 75 * 2 * 150.0
    g = np.float32(S / np.sqrt(2 * 19200.0))
    assert len(LR.dd_errors(LR.fresh_state(), rows(0.03), float(g))) == 2


def _oracle_frames(fr, n):
    return [dict(start=int(r["start"]), flags=int(r["flags"]), peak_to_mean=np.float32(r["peak_to_mean"])) for r in fr[:n]]


class _Capture:
    """Stands for a whole capture of which only the last locked frame's first 4096 samples are ever read."""

    def __init__(self, start, level):
        self.start, self.level = start, level

    def __getitem__(self, sl):
        assert sl.start == self.start and sl.stop == self.start + 4096
        return self.level


def test_oracle_under_the_same_bars_sensitivity_and_ambiguity(built):
    """On the inputs of every GPU case (synthetic arrays of the same shapes): the reference's outcome is unambiguous
    except in edge_* cases, no budget exceeds the bar test_tracking.check_state uses, oracle.stream_update / track_update /
    dd_loop_error land inside the budgets, and a frame's entries dropped or counted twice (a locked slot's residual
    dropped) move the reference by more than 4 budgets."""
    from oracle import oracle as O
    for case in stream_cases():
        for s, (state, rows, x) in enumerate(stream_synthetic(case)):
            what = ("stream", case["name"], case["dd"], s)
            outs = LR.stream_update(state, rows, x, 0.9, dd=bool(case["dd"]), dd_gate=case["gate"])
            assert len(outs) == 1, what
            check_budgets(outs, what)
            got = O.stream_update(f32_state(state), rows, x, 0.9, dd=bool(case["dd"]), dd_gate=case["gate"])
            frac = LR.accept(got, outs, fields=set(got))
            note("oracle stream", frac, 1, 1)
            F = rows.shape[0]
            o = outs[0]
            assert o["wrap_edge"] is False
            if case["name"] == "wrap":
                assert abs(o["fine_freq_offset"]) > 0.4 / 2048 and o["fine_freq_offset"] * state["fine_freq_offset"] < 0, what
            for f in (range(F) if F > 1 else ()):
                for alt in (np.delete(rows, f, axis=0), np.concatenate([rows, rows[f:f + 1]])):
                    (m,) = LR.stream_update(state, alt, x, 0.9, dd=bool(case["dd"]), dd_gate=case["gate"])
                    assert abs(m["last_fine_error"] - o["last_fine_error"]) > 4 * o["d_err"], (what, f)
    for case in list(tracked_size_cases()) + list(tracked_edge_cases()):
        for s, (state, fr, rows, x) in enumerate(tracked_synthetic(case)):
            what = ("tracked", case["name"], s, case["streams"][s].get("name"))
            assert not LR.position_ties(state, case["streams"][s]["j0"], case["C"]), what
            outs, count = tracked_reference(case, state, fr, rows, x)
            assert count == case["C"] and len(outs) == 1, what
            check_budgets(outs, what)
            o = outs[0]
            locked = [i for i in range(count) if fr[i]["flags"] == 3]
            cap = _Capture(int(fr[locked[-1]]["start"]), x) if locked else None
            got, ocount = O.track_update(f32_state(state), _oracle_frames(fr, count), rows[:count], cap, case["n_samples"], case["MF"],
                                         case["advance"], dd=bool(case["dd"]), dd_gate=case["gate"])
            assert ocount == count
            note("oracle tracked", LR.accept(got, outs, fields=set(got)), 1, 1)
            n = len(locked)
            if n >= 2 and o["steers"]:
                for f in locked:
                    for keep in ([i for i in locked if i != f], locked + [f]):
                        r2 = rows.copy()
                        fr2 = fr.copy()
                        if len(keep) < n:
                            fr2["flags"][f] = 2
                            (m,), _ = tracked_reference(case, state, fr2, rows, x)
                            assert max(abs(m["alpha"] - o["alpha"]) / o["d_alpha"], abs(m["slope"] - o["slope"]) / max(o["d_slope"], 1e-300)) > 4, (what, f)
                            e2 = m["last_fine_error"]
                        else:                                     # the frame's entries counted twice: by the fine loop alone
                            alt = np.concatenate([rows[locked], rows[f:f + 1]])
                            e2 = LR.fine_loop(state, alt, x, n + 1, 0.9, dd=bool(case["dd"]), dd_gate=case["gate"])[0]["last_fine_error"]
                        if f != locked[-1] or len(keep) > n:      # (dropping the last locked frame also moves the level's frame)
                            assert abs(e2 - o["last_fine_error"]) > 4 * o["d_err"], (what, f, len(keep))
    for name, fr, cnt, state in start_streams():
        o = LR.track_start(state, fr, cnt, START_MF, 3 * L)
        check_budgets([o], name)
        n = min(cnt, START_MF)
        recs = [types.SimpleNamespace(start=int(r["start"]), flags=int(r["flags"]), fine_offset=np.float32(r["fine_offset"]),
                                      coarse_carriers=int(r["coarse_carriers"]), peak_to_mean=np.float32(r["peak_to_mean"])) for r in fr[:n]]
        got = O.track_start(f32_state(state), recs, 3 * L)
        note("oracle start", LR.accept(got, [o], fields=set(got)), 1, 1)
    for g in ("oracle stream", "oracle tracked", "oracle start"):
        show(g)


def test_edge_cases_sit_on_their_thresholds():
    """edge_*: inputs built to sit on a threshold return both outcomes, each with its own consequences."""
    rng = np.random.default_rng(3)
    rows = synth_rows(rng, np.array([0.02, -0.03]), 1.0, 0)
    x = synth_level(rng, 1.0)
    lv, _ = LR.level_of(x)
    # edge_level: the average is the level / thr to the last float32
    avg = float(np.float32(lv / float(np.float32(0.35))))
    outs = LR.stream_update(LR.fresh_state(signal_average=avg), rows, x, 0.9)
    assert sorted(o["level_lost"] for o in outs) == [False, True]
    assert {o["total_frames_desync"] for o in outs} == {0, 1} and {o["signal_average"] == avg for o in outs} == {True, False}
    # edge_wrap: the new fine offset falls on +half a carrier: compared modulo one carrier
    err = LR.cp_error(rows)[0]
    fine = float(np.float32(LR.HALF + 0.9 * err))
    (o,) = LR.stream_update(LR.fresh_state(fine_freq_offset=fine), rows, x, 0.9)
    assert o["wrap_edge"]
    assert LR.accept(dict(o, fine_freq_offset=o["fine_freq_offset"] - np.sign(o["fine_freq_offset"]) / 2048.0), [o]) is not None
    # edge_branch: e_cp - e_dd half a step apart: both branches, each with its own error
    r = np.zeros((2, 76), np.complex128)
    r[:, 1:] = 150.0 * np.exp(0.3j)
    e_dd = (0.3 - np.pi) * LR.K_DD
    r[:, 0] = 300.0 * np.exp(2j * np.pi * 2048 * (e_dd + 0.5 * LR.STEP))
    outs = LR.dd_errors(LR.fresh_state(), r, 2.5)
    assert sorted(o["dd_branch"] for o in outs) == [0, 1] and abs(outs[0]["err"] - outs[1]["err"]) > 0.9 * LR.STEP


# ======================================================================================================== GPU
@pytest.fixture(scope="module")
def lctx(built):
    from conftest import make_ctx
    c = make_ctx(None, 512)
    yield c
    c.set_stream_loop(decision_directed=False)
    c.close()


@pytest.fixture(scope="module")
def base_frames(built, ensemble_iq):
    """The five frames of one ensemble from their null symbols, on the device: [5][196608]."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(ensemble_iq)).to(torch.device("cuda", 0))


def read_states(torch, ctx, n):
    import dabgpu
    ctx.sync()
    t = dabgpu.device_tensor(torch, ctx.stream_states_ptr, (n * 64,), torch.uint8, torch.device("cuda", 0))
    return t.cpu().numpy().view(dabgpu.STREAM_STATE_DTYPE).copy()


def write_states(torch, ctx, states):
    """Prior states through dabgpu_stream_states, as a caller seeding them would."""
    import dabgpu
    rec = np.zeros(len(states), dabgpu.STREAM_STATE_DTYPE)
    for i, st in enumerate(states):
        for k, v in LR.fresh_state(**st).items():
            rec[i][k] = v
    ctx.sync()
    t = dabgpu.device_tensor(torch, ctx.stream_states_ptr, (len(states) * 64,), torch.uint8, torch.device("cuda", 0))
    t.copy_(torch.from_numpy(rec.view(np.uint8).copy()))
    torch.cuda.synchronize()


def rotate(torch, x, cfo, amp):
    """x [k][n] times amp exp(2 pi j cfo_k n): the phase formed in float64."""
    n = torch.arange(x.shape[1], dtype=torch.float64, device=x.device)
    ph = torch.remainder(cfo.to(torch.float64)[:, None] * n[None, :], 1.0) * (2 * np.pi)
    return x * torch.polar(torch.full_like(ph, amp, dtype=torch.float32), ph.to(torch.float32))


def noise(torch, shape, sigma, gen, dev):
    return sigma * torch.view_as_complex(torch.randn(tuple(shape) + (2,), generator=gen, device=dev, dtype=torch.float32))


def build_stream_iq(torch, base, case):
    """[S * F][stride] on the device: frames of the ensemble gathered, rotated by the stream's offset plus the frame's
    own residual, generator noise at 20 dB."""
    dev = base.device
    S, F, stride = len(case["streams"]), case["F"], case["stride"]
    iq = torch.zeros((S * F, stride), dtype=torch.complex64, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(case["seed"])
    frames = base[:, NULL:NULL + SYMS]
    for s, st in enumerate(case["streams"]):
        for f0 in range(0, F, 24):
            f1 = min(F, f0 + 24)
            idx = torch.arange(f0 + s, f1 + s, device=dev) % 5
            cfo = torch.from_numpy((st["c"] + st["delta"][f0:f1]) / 2048.0).to(dev)
            iq[s * F + f0:s * F + f1, :SYMS] = rotate(torch, frames[idx], cfo, st["amp"]) + \
                noise(torch, (f1 - f0, SYMS), 0.1 * st["amp"] * np.sqrt(0.5), gen, dev)
    return iq


def run_stream_case(lctx, base_frames, case):
    import torch
    import dabgpu
    dev = base_frames.device
    S, F, stride, dd = len(case["streams"]), case["F"], case["stride"], case["dd"]
    iq = build_stream_iq(torch, base_frames, case)
    soft = torch.zeros((S * F, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
    rows_t = torch.zeros((S * F, 76), dtype=torch.complex64, device=dev)
    lctx.streams_reset(S)
    lctx.set_stream_loop(decision_directed=bool(dd))
    lctx.set_loop_gate(case["gate"])
    write_states(torch, lctx, [st["pre"] for st in case["streams"]])
    before = read_states(torch, lctx, S)
    if dd:                                                        # the sums of the same samples at the pre-call offset
        fo = np.repeat((before["fine_freq_offset"] + before["coarse_freq_offset"]).astype(np.float32), F)
        d_fo = torch.from_numpy(fo).to(dev)
        torch.cuda.synchronize()
        lctx.ofdm_demod_frames_dd_dev(iq.data_ptr(), stride, S * F, d_fo.data_ptr(), soft.data_ptr(), rows_t.data_ptr())
        lctx.ofdm_demod_streams_dev(iq.data_ptr(), stride, S, F, 0.9, soft.data_ptr(), None, None)
    else:
        torch.cuda.synchronize()
        lctx.ofdm_demod_streams_dev(iq.data_ptr(), stride, S, F, 0.9, soft.data_ptr(), rows_t.data_ptr(), None)
    after = read_states(torch, lctx, S)
    rows = rows_t.cpu().numpy().reshape(S, F, 76)
    last = iq[F - 1::F, :4096].cpu().numpy()
    group = "stream call %s" % ("dd" if dd else "cp")
    for s in range(S):
        state = LR.state_of(before[s])
        assert state["fine_freq_offset"] == case["streams"][s]["pre"]["fine_freq_offset"]
        outs = LR.stream_update(state, rows[s], last[s], 0.9, dd=bool(dd), dd_gate=case["gate"],
                                ds_input=LR.dd_input(F * LR.TERMS_PER_FRAME) if dd else 0.0)
        what = (case["name"], dd, s)
        assert len(outs) == 1, what                               # (no stream case is an edge case)
        o = outs[0]
        if s == 2:
            assert o["level_lost"] and o["steers"] == (F > 1), what
        else:
            assert not o["level_lost"], what
        if case["name"] == "wrap":
            assert o["fine_freq_offset"] * state["fine_freq_offset"] < 0 and not o["wrap_edge"], what
        if dd:
            assert not o.get("gated") and o["dd_branch"] == 0, what
        try:
            frac = LR.accept(after[s], outs)
        except AssertionError as e:
            raise AssertionError("%r: %s" % (what, e))
        note(group, frac, 1, 1)
    return group


@pytest.mark.gpu
@pytest.mark.parametrize("dd", [0, 1])
@pytest.mark.parametrize("name", ["F%d" % F for F in SIZES] + ["wrap"])
def test_gpu_stream_call_state_against_the_reference(lctx, base_frames, name, dd):
    """dabgpu_ofdm_demod_streams_dev at 1 .. 216 frames per stream (three streams with their own offsets, levels and prior
    states up to 14 frames, two from 107 on; `wrap`: two frames, a padded frame_stride, fine offsets pushed over +half and
    -half a carrier), both estimators: the state after the call within the reference's budgets of what the definition gives
    for the state before and the call's own correlations / fourth-power sums."""
    case = next(c for c in stream_cases() if c["name"] == name and c["dd"] == dd)
    show(run_stream_case(lctx, base_frames, case))


def build_capture(torch, base, case):
    """[S][n_samples]: noise at -20 dB of the stream's level; frame i of the ensemble where the stream's slot i lies (its
    PRS prefix 64 samples behind the record's start), rotated by the stream's offset plus its own residual -- the
    frequency steps fall into the null symbols; an unlocked slot holds noise of the stream's level instead."""
    dev = base.device
    S, C, n = len(case["streams"]), case["C"], case["n_samples"]
    gen = torch.Generator(device=dev)
    gen.manual_seed(case["seed"])
    x = torch.empty((S, n), dtype=torch.complex64, device=dev)
    frames = base[:, NULL:NULL + SYMS]
    for s, st in enumerate(case["streams"]):
        for a in range(0, n, 1 << 24):
            b = min(n, a + (1 << 24))
            x[s, a:b] = noise(torch, (b - a,), 0.1 * st["amp"] * np.sqrt(0.5), gen, dev)
        for i in range(C):
            p = int(st["pos"][i]) + MARGIN
            if i in st["unlocked"]:
                x[s, p - 2000:p + SYMS] = noise(torch, (SYMS + 2000,), st["amp"] * np.sqrt(0.5), gen, dev)
            else:
                cfo = torch.tensor([(st["c"] + st["delta"][i]) / 2048.0], device=dev)
                x[s, p:p + SYMS] += rotate(torch, frames[(i + s) % 5][None, :], cfo, st["amp"])[0]
    return x


def sync_records_against_reference(case, s, state, cap, fr, count, cfg):
    """Every frame record of a small tracked call against sync_reference.Sync at the reference's predicted candidate."""
    import sync_reference as SR
    j0, slots, _ = LR.predict(state, case["n_samples"], case["MF"])
    assert len(slots) == count
    f = np.float32(np.float32(state["fine_freq_offset"]) + np.float32(state["coarse_freq_offset"]))
    n_unamb = 0
    worst = 0.0
    for i, cand in enumerate(slots):
        sy = SR.Sync(cap[cand:cand + 2552], f, 0, expected=cfg.timing_margin, distance_prob=cfg.impulse_peak_distance_probability,
                     first_path_rel=cfg.first_path_rel)
        tp = sy.taps(0)
        r = fr[i]
        what = (case["name"], s, i)
        t = int(r["start"]) - cand + cfg.timing_margin
        assert (t % SR.N) in tp.accepted, (what, t, sy.t)
        if tp.unambiguous:
            assert t == sy.t, (what, t, sy.t)
        n_unamb += bool(tp.unambiguous)
        errs = [abs(float(r["peak_to_mean"]) - v) / b for v, b in tp.ptm_of.values()]
        assert min(errs) <= 1.0, (what, float(r["peak_to_mean"]), sy.ptm, min(errs))
        worst = max(worst, min(errs))
        ptm, dptm = tp.ptm_of[tp.peak]
        start = int(r["start"])
        inside = start >= 0 and start + SYMS <= case["n_samples"]
        assert bool(r["flags"] & 2) == inside, what
        assert SR.threshold_ok(ptm, dptm, float(np.float32(cfg.min_peak_to_mean)), r["flags"] & 1), (what, ptm, int(r["flags"]))
        assert float(r["freq_offset"]) == float(f) and float(r["fine_offset"]) == float(np.float32(state["fine_freq_offset"])), what
        if i not in case["streams"][s]["unlocked"]:
            assert tp.unambiguous and abs(start - int(case["streams"][s]["pos"][i])) <= 1, (what, start)
    note("MODE_TRACK records", {"peak_to_mean": worst}, n_unamb, count)


def run_tracked_case(lctx, base_frames, case, check_sync=False):
    import torch
    import dabgpu
    dev = base_frames.device
    S, C, MF, n = len(case["streams"]), case["C"], case["MF"], case["n_samples"]
    dd = case["dd"]
    x = build_capture(torch, base_frames, case)
    frames_t = torch.zeros((S, MF, 32), dtype=torch.uint8, device=dev)
    counts_t = torch.zeros(S, dtype=torch.int32, device=dev)
    soft = torch.zeros((S * MF, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
    rows_t = torch.zeros((S * MF, 76), dtype=torch.complex64, device=dev)
    cfg = dabgpu.track_cfg(decision_directed=dd, dd_gate=case["gate"])
    lctx.streams_reset(S)
    write_states(torch, lctx, [st["state"] for st in case["streams"]])
    before = read_states(torch, lctx, S)
    torch.cuda.synchronize()
    lctx.ofdm_demod_tracked_dev(x.data_ptr(), n, S, n, MF, case["advance"], soft.data_ptr(), frames_t.data_ptr(), counts_t.data_ptr(),
                                cfg=cfg, d_cyc=None if dd else rows_t.data_ptr())
    after = read_states(torch, lctx, S)
    fr = frames_t.cpu().numpy().view(dabgpu.ACQUIRED_FRAME_DTYPE).reshape(S, MF)
    cnt = counts_t.cpu().numpy()
    if dd:                                                        # the sums of the frames the call found, at the offset it applied
        locked = [(s, i) for s in range(S) for i in range(C) if (fr[s, i]["flags"] & 3) == 3]
        g = torch.stack([x[s, int(fr[s, i]["start"]):int(fr[s, i]["start"]) + SYMS] for s, i in locked]).contiguous()
        d_fo = torch.from_numpy(np.array([fr[s, i]["freq_offset"] for s, i in locked], np.float32)).to(dev)
        sums = torch.zeros((len(locked), 76), dtype=torch.complex64, device=dev)
        torch.cuda.synchronize()
        lctx.ofdm_demod_frames_dd_dev(g.data_ptr(), SYMS, len(locked), d_fo.data_ptr(), soft.data_ptr(), sums.data_ptr())
        lctx.sync()
        for k, (s, i) in enumerate(locked):
            rows_t[s * MF + i] = sums[k]
    rows = rows_t.cpu().numpy().reshape(S, MF, 76)
    group = "tracked call %s" % ("dd" if dd else "cp")
    for s, st in enumerate(case["streams"]):
        what = (case["name"], s, st.get("name"))
        state = LR.state_of(before[s])
        assert not LR.position_ties(state, st["j0"], C), what
        assert cnt[s] == C, (what, cnt[s])
        plan = [i for i in range(C) if i not in st["unlocked"]]
        got_locked = [i for i in range(C) if (fr[s, i]["flags"] & 3) == 3]
        assert got_locked == plan, (what, got_locked, plan)       # (the case is what it says: the planned slots locked, no others)
        level = None
        if plan:
            p = int(fr[s, plan[-1]]["start"])
            level = x[s, p:p + 4096].cpu().numpy()
        n_locked = len(plan)
        outs, count = tracked_reference(case, state, fr[s], rows[s], level,
                                        ds_input=LR.dd_input(n_locked * LR.TERMS_PER_FRAME) if dd else 0.0)
        assert count == C and len(outs) == 1, (what, len(outs))
        try:
            frac = LR.accept(after[s], outs)
        except AssertionError as e:
            raise AssertionError("%r: %s" % (what, e))
        note(group, frac, 1, 1)
        edge_expectations(st.get("name"), case, state, outs[0], after[s])
        if check_sync:
            sync_records_against_reference(case, s, state, x[s].cpu().numpy(), fr[s], C, cfg)
        assert (fr[s, C:]["flags"] == 0).all() and (fr[s, C:]["start"] == -1).all(), what
    return group


def edge_expectations(name, case, state, o, after):
    """What each edge case is there for, asserted on the reference's outcome (the device state was held to it)."""
    if name is None:
        return
    if name in ("none_locked", "none_of_one"):
        assert o["tracking"] == 0 and int(after["tracking"]) == 0 and o["total_frames_desync"] == state["total_frames_desync"] + case["C"]
    else:
        assert o["tracking"] == 1
    if name == "one_of_one":
        assert o["drift"] != state["drift"] and o["slope"] == 0.0
    if name == "one_of_several":
        assert o["drift"] == state["drift"]
    if name == "skipped_samples":
        assert o["total_frames_desync"] == state["total_frames_desync"] + 2 + 1
    if name == "level_lost_several":
        assert o["level_lost"] and o["steers"] and o["signal_average"] == state["signal_average"] and o["fine_freq_offset"] != state["fine_freq_offset"]
    if name == "level_lost_single":
        assert o["level_lost"] and not o["steers"] and o["fine_freq_offset"] == state["fine_freq_offset"] and o["total_frames_read"] == state["total_frames_read"]
    if name == "no_average_yet":
        assert o["signal_average"] == o["level"]
    if name in ("wrap_plus", "wrap_minus"):
        assert o["fine_freq_offset"] * state["fine_freq_offset"] < 0 and abs(o["fine_freq_offset"]) > 0.4 / 2048
    if case["dd"] and case["gate"] > 100:
        if o["steers"]:
            assert o["loop_gated"] == state["loop_gated"] + 1 and o["dd_pending"] == NOB
    elif name == "dd_after_start":
        assert state["dd_branch"] == NOB and o["dd_branch"] == 0 and o["loop_gated"] == state["loop_gated"]
    elif name == "dd_branch_held":
        assert (o["dd_branch"], o["dd_pending"], o["loop_gated"]) == (0, 1, state["loop_gated"] + 1)
    elif name == "dd_branch_believed":
        assert (o["dd_branch"], o["dd_pending"], o["loop_gated"]) == (1, NOB, state["loop_gated"])
    elif name == "dd_level_lost":                                 # one locked frame, its level lost: the gate's memory stays
        assert not o["steers"] and (o["dd_pending"], o["loop_gated"]) == (1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("C", SIZES)
def test_gpu_tracked_call_state_against_the_reference(lctx, base_frames, C):
    """dabgpu_ofdm_demod_tracked_dev with 1 .. 216 slots inside the capture, clocks off by +-60-150 ppm, every frame at its own
    residual offset, unlocked slots (noise) at the first, the last and slots 13, 107, 108 beside random ones: counts, frame
    slots and the state after the call against the reference; up to 14 slots every frame record against sync_reference."""
    case = next(c for c in tracked_size_cases() if c["C"] == C)
    show(run_tracked_case(lctx, base_frames, case, check_sync=C <= 14))
    show("MODE_TRACK records")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges5", "edges1", "edges_dd", "edges_dd_gated"])
def test_gpu_tracked_call_edges_against_the_reference(lctx, base_frames, name):
    """The tracked call's rules at small counts, one stream each in a shared call: nothing locks; one of one; one of
    several; 2, 3, 4, 5 locked (the gain's steps); samples skipped (j0 = 2); the last locked frame's level lost with one and
    with several locked; no average yet; wraps at +-half a carrier; decision-directed: first call after a start, locked,
    a branch departure held and then believed, a lost level leaving the gate's memory alone, and everything gated by quality."""
    case = next(c for c in tracked_edge_cases() if c["name"] == name)
    show(run_tracked_case(lctx, base_frames, case, check_sync=(name == "edges1")))


@pytest.mark.gpu
@pytest.mark.parametrize("only_lost", [0, 1])
def test_gpu_track_start_against_the_reference(lctx, only_lost):
    """dabgpu_track_start_dev on synthetic acquisition records (no IQ): 1 .. 130 records with one and two missed frames and
    +-2 samples of jitter, unlocked records at both ends, none locked, counts[s] above max_frames; streams that are and are
    not tracking, only_lost 0 and 1."""
    import torch
    dev = torch.device("cuda", 0)
    streams = start_streams()
    S = len(streams)
    adv = 3 * L
    frames_t = torch.from_numpy(np.stack([fr for _, fr, _, _ in streams]).view(np.uint8).copy()).to(dev)
    counts_t = torch.from_numpy(np.array([c for _, _, c, _ in streams], np.int32)).to(dev)
    lctx.streams_reset(S)
    write_states(torch, lctx, [st for _, _, _, st in streams])
    before = read_states(torch, lctx, S)
    torch.cuda.synchronize()
    lctx.track_start_dev(frames_t.data_ptr(), counts_t.data_ptr(), S, START_MF, adv, only_lost=bool(only_lost))
    after = read_states(torch, lctx, S)
    for s, (name, fr, cnt, _) in enumerate(streams):
        o = LR.track_start(LR.state_of(before[s]), fr, cnt, START_MF, adv, only_lost=bool(only_lost))
        if only_lost and o["tracking"] == 2:
            o["tracking"] = 1                                     # (a stand-alone start settles its own marks: dabgpu.h)
        try:
            frac = LR.accept(after[s], [o])
        except AssertionError as e:
            raise AssertionError("%s only_lost %d: %s" % (name, only_lost, e))
        note("track_start", frac, 1, 1)
    show("track_start")


@pytest.mark.gpu
def test_gpu_frame_call_coarse_and_fine_against_the_reference(lctx, ensemble_iq):
    """dabgpu_ofdm_demod_stream_frame, three frames of one stream: acquiring (the coarse offset is stored), not acquiring
    on the same carrier (nothing moves it), then a frame one carrier further (the slow update: coarse_freq_slow_beta x
    k^ / 2048).  After each frame that is not acquiring the fine loop's state against the reference, fed the correlations
    of the same frame at the offset the call applied."""
    import dabgpu
    M = 128
    cfg = dabgpu.track_cfg(timing_margin=M, min_peak_to_mean=100.0)
    rng = np.random.default_rng(21)
    import torch
    lctx.streams_reset(1)
    for f, (cfo, acquiring) in enumerate(((2.27, True), (2.30, False), (3.24, False))):
        frame = synth.channel(ensemble_iq[f], snr_db=18.0, cfo=cfo / 2048.0, rng=rng)[NULL - M:NULL - M + SYMS]
        before = LR.state_of(read_states(torch, lctx, 1)[0])
        soft, res, _ = lctx.ofdm_demod_stream_frame(frame, 0, acquiring=acquiring, cfg=cfg)
        after = LR.state_of(read_states(torch, lctx, 1)[0])
        k = int(res.sync.coarse_carriers)
        assert res.flags == 3 and k == (2, 0, 1)[f], (f, k, res.flags)
        coarse, dco = LR.coarse_update(before["coarse_freq_offset"], k, True, acquiring, cfg.max_coarse_carriers, cfg.coarse_freq_slow_beta)
        assert abs(after["coarse_freq_offset"] - coarse) <= dco, (f, after["coarse_freq_offset"], coarse)
        if f == 2:
            assert dco > 0 and abs(coarse + (2.0 + 0.1) / 2048) < 1e-9
        assert after["total_frames_read"] == f + 1 and after["total_frames_desync"] == 0
        if acquiring:
            continue
        applied = np.float32(np.float32(before["fine_freq_offset"]) + np.float32(after["coarse_freq_offset"]))
        _, cyc, _ = lctx.ofdm_demod_frames(frame[None, :], np.array([applied], np.float32), want_cyc=True)
        rec = np.zeros(1, FRAME_DTYPE)
        rec["flags"], rec["peak_to_mean"] = res.flags, res.sync.peak_to_mean
        outs, _ = LR.track_update(dict(before, coarse_freq_offset=after["coarse_freq_offset"]), rec, cyc, frame[:4096], SYMS, 1, 0,
                                  fine_beta=cfg.fine_freq_update_beta, signal_beta=cfg.signal_update_beta,
                                  thr_null_start=cfg.thr_null_start, fixed_start=True)
        assert len(outs) == 1
        note("frame call", LR.accept(after, outs), 1, 1)
    show("frame call")
