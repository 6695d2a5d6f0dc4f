"""The frequency and timing loops (SURVEY.md 8f-1, row A2's closed loop) restated from include/dabgpu.h ("closed-loop
front end", dabgpu_track_cfg, dabgpu_set_stream_loop, dabgpu_set_loop_gate, dabgpu_stats) and the prose of csrc/kernels.hpp
(StreamState, dd_loop_error, launch_track_start, TrackUpdateArgs), in float64 / complex128 (the timing line in extended
precision), for the tests of the state machines behind dabgpu_ofdm_demod_streams_dev, dabgpu_ofdm_demod_tracked_dev,
dabgpu_ofdm_demod_stream_frame and dabgpu_track_start_dev.  Written without oracle/, dab_tables.hpp or the library.

Definitions.  A state is the 64-byte dabgpu_stream_state.  K_CP = 1 / (2 pi 2048), K_DD = 1 / (4 2 pi 2552),
STEP = 1 / (4 2552) (0.2 carriers), HALF = 0.5 / 2048 (half a carrier); cfg values are the float32 the ABI carries.

Stream call (frames consecutive frames of one stream, entry [f][l] the call's loop input):
- err = (mean over all frames x 76 entries of angle(entry)) K_CP.
- level = mean over the first 4096 samples of the stream's LAST frame of |re| + |im|.
- level_lost = signal_average > 0 and level < thr_null_start signal_average.
- steers = not (level_lost and frames == 1): a single frame whose level is lost steers nothing.
- steers: fine = fine - beta err, then + one carrier where it fell below -HALF, - one carrier where above +HALF.
- last_fine_error = err in either case.
- level_lost: total_frames_desync += 1, total_frames_read += frames - 1, the average stays.  Otherwise
  total_frames_read += frames and signal_average = signal_beta average + (1 - signal_beta) level, or = level while the
  average is still 0 (the first-value rule).
Decision-directed variant (entries 1..75 hold fourth-power sums, entry 0 the PRS's cyclic-prefix correlation):
- S = sum of the entries 1..75 of every frame; n_terms = frames x terms_per_frame (19200: 256 carriers x 75 symbols).
- e_cp = (mean over the frames of angle(entry 0)) K_CP.
- quality gate: n_terms <= 0 or |S|^2 < gate^2 n_terms -> err = e_cp, dd_branch = rint(e_cp / STEP), dd_pending = none,
  loop_gated += 1.
- otherwise e_dd = angle(-S) K_DD, k = rint((e_cp - e_dd) / STEP).  Branch hold: not the first call (total_frames_read
  != 0), dd_branch == 0, k = +-1 and dd_pending != k -> dd_pending = k, loop_gated += 1, k = 0; else dd_pending = none.
  dd_branch = k, err = e_dd + k STEP.
- an estimate that is not applied (steers false) leaves loop_gated, dd_branch and dd_pending alone; last_fine_error is
  still the estimate.  After a start (track_start) dd_branch = dd_pending = DD_NO_BRANCH: nothing is held.

Tracked call's prediction: period = 196608 + drift; j0 = the number of frames that lie before the capture, the j >= 0
with next_frame_start + j period < 0; slot i sits at rint(next_frame_start + (j0 + i) period); the list ends at the
first slot that does not fit (0 <= slot and slot + 76 2552 + 512 <= n_samples) and at max_frames: count slots.

Tracked call's update (frames[i], i < count, the call's frame records; locked = both flag bits set):
- the fine loop above over the locked frames' entries, with n locked frames in place of `frames` and the level of the
  LAST locked frame (its first 4096 samples from frames[last].start).
- residuals r_i = start_i - p_i against the unrounded prediction p_i = next + (j0 + i) period.
- n >= 2: the least-squares line r = alpha + slope i; drift += drift_beta min(1, n / 4) slope.
- n == 1: alpha = r, slope = 0; drift += drift_beta 0.125 r when count == 1, else drift stays.
- next_frame_start = p(count) + alpha + slope count - advance (p with the OLD drift).
- n >= 1: last_time_offset = start_last - rint(p_last), last_peak_to_mean = the last locked frame's.
- total_frames_read += n (one less when the level is lost), total_frames_desync += j0 + (count - n) (one more when the
  level is lost); count > 0 and n == 0: tracking = 0.
- frame call (fixed start): one slot at sample 0, no timing update, no j0.  Before the fine loop the PRS search moves
  the coarse offset when it ran (max_coarse_carriers > 0) and the frame locked: acquiring: coarse = -k^ / 2048 (and the
  fine offset is set from the PRS's prefix); otherwise, k^ != 0: coarse -= coarse_freq_slow_beta k^ / 2048.

track_start (count = min(counts[s], max_frames) acquisition records):
- only_lost and the stream is tracking (1): nothing changes.  No locked record: tracking = 0, nothing else changes.
- j_i = round((start_i - start_first) / 196608) for the locked records; slope of the least-squares line start against
  j; drift = slope - 196608 with four or more locked records, else 0.
- next_frame_start = start_last + 196608 + drift (as stored: float32) - advance; fine = mean of the locked records'
  fine offsets; coarse = -coarse_carriers_last / 2048; tracking = 2 when only_lost else 1; dd_branch = dd_pending =
  DD_NO_BRANCH; total_frames_read += n; last_time_offset = 0; last_peak_to_mean = the last locked record's.

Error budgets.  u = 2^-24; like sync_reference and ofdm_reference each is the forward-error bound of a correct float32
implementation of the same definition (Higham, 2nd ed., section 4.2: a sum of n terms in any order whose longest chain
of additions is D has |error| <= gamma_D sum |x_i|; half an ulp = u relative for every float32 result).
- D(n) = ceil(n / 1024) + 22: the loops are one 1024-thread workgroup per stream (kernels.hpp), so a thread adds
  ceil(n / 1024) terms and the partial sums meet in at most 22 more additions (a six-level wave tree and sixteen waves
  in sequence; a ten-level tree is shorter).  A plain sequential sum of 16416 terms (gamma_16415 = 1e-3) is NOT inside
  this budget -- it would miss the 2e-9 bar by an order of magnitude.
- C_ATAN2 = 12: the relative error, in u, of a float32 atan2.  HIP's table of device-function accuracy is not part of
  this repository or its toolchain's installed documents; the source used is the OpenCL 3.0 specification, section
  7.4 (relative error as ULPs, full profile): atan2 <= 6 ulp, which the ROCm device library's atan2 is written to, and
  one ulp is at most 2 u of the value.  (HIP's own table, where available, lists a smaller figure; 12 u bounds both.)
- angle mean m over n angles divided by q: dm = (C_ATAN2 u + gamma_D(n)) sum |angle| / q + u |m|; err = m K_CP:
  derr = dm K_CP + 2 u |err| (the constant's rounding and the product's).
- fine: dfine = beta derr + u |beta err| + u |fine'| (+ u |fine''| after a wrap).
- level: 8192 absolute values: dlevel = (gamma_32 + u) level (eight per thread and 22 more, then the exact 2^-12).
  The threshold product: 2 u thr average.  signal_average: (1 - signal_beta) dlevel + 4 u average' (1 - beta is exact by
  Sterbenz for beta >= 0.5; two products and a sum); first value: dlevel.
- S: dS = gamma_D(n) sum (|re| + |im|) of the entries (+ the input term below); |S|^2: 2 |S| dS + dS^2 + 3 u |S|^2,
  the threshold gate^2 n_terms: 2 u of it.  angle(-S): dang = asin(min(1, dS / |S|)) + C_ATAN2 u |ang|;
  e_dd: dang K_DD + 2 u |e_dd|.  v = (e_cp - e_dd) / STEP: dv = (de_cp + de_dd) / STEP + 3 u |v|.
  err = e_dd + k STEP: de_dd + u |k| STEP + u |err|.
- dd_input(n_terms) = gamma_85 n_terms: where a test regenerates the fourth-power sums with a second launch, that
  launch may cut its frames into other runs; ofdm_reference's dd4 budget gives a run's sum gamma_(10 + symbols) of its
  unit terms.  Added to dS by the caller, 0 otherwise.
- timing: next_frame_start is a double in the ABI and positions reach 4e7 samples, beyond float32's integers; the
  line is float64 arithmetic by definition and its budget uses u64 = 2^-53 with the same bounds (the reference itself
  runs in extended precision).  dr_i = 2 u64 |p_i| + u64 |r_i|; with R_i = |r_i| + dr_i and the exact integer
  det = n sum i^2 - (sum i)^2: dslope = (gamma64_(n+3) (n sum i R_i + sum i sum R_i) + n sum i dr_i + sum i sum dr_i) /
  det + 3 u64 |slope|; dalpha = (gamma64_n sum R + sum dr + dslope sum i + 2 u64 |slope sum i|) / n + 2 u64 |alpha|;
  dnext = dalpha + count dslope + 4 u64 max(|p(count)|, |advance|, |next'|).
  drift is stored as float32: ddrift = gain dslope^ + u |drift'|.
- track_start: every sum of the line is an integer below 2^53, exact in float64; the quotient and the difference carry
  4 u64 196608, the stored drift u |drift|; next: ddrift + 4 u64 |start_last|; fine: (gamma_D(n) + u) mean |fine_i|.
No budget comes out above the bars test_tracking.check_state holds against the oracle (2e-9 fine and error, 1e-4
samples next_frame_start, 1e-5 relative drift and level): the test file asserts it on every case.  The old bars were
not vacuous: the fine offset's bar is some ten to thirty budgets wide at the sizes of this file, and a frame's entries
dropped or counted twice move the error by more than that bar as well; what the comparison with the oracle lacked was
the sizes and an independent definition, not a tighter bar.

Discrete outcomes (level_lost, the quality gate, the branch k, the wrap).  Following sync_reference's acceptance rule, an
outcome is exact unless the reference value lies within its budget of the threshold or of a rounding tie; there every
outcome is returned, each with its own consequences, and a case is UNAMBIGUOUS when one outcome is returned.  The wrap
is not an alternative: where the unwrapped fine offset lies within its budget of +-HALF the outcome says so (wrap_edge)
and fine offsets are compared modulo one carrier; everywhere else exactly.  The >= 4 records rule counts integers.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
C_ATAN2 = 12.0                                                   # beside ofdm_reference's C_FFT, C_NCO: see the docstring
NB_FFT, NB_SYM, NB_SYMBOLS = 2048, 2552, 76
L_FRAME = 196608
FRAME_LEN = NB_SYMBOLS * NB_SYM
FIT_SLACK = 512
LEVEL_SAMPLES = 4096
K_CP = 1.0 / (2.0 * math.pi * NB_FFT)
K_DD = 1.0 / (4.0 * 2.0 * math.pi * NB_SYM)
STEP = 1.0 / (4.0 * NB_SYM)
HALF = 0.5 / NB_FFT
DD_NO_BRANCH = 0x7fffffff
TERMS_PER_FRAME = 256 * 75
LD = np.longdouble

# the bars test_tracking.check_state holds against the oracle
BAR_FINE, BAR_NEXT, BAR_REL = 2e-9, 1e-4, 1e-5


def gamma(n, u=U):
    return n * u / (1.0 - n * u)


def depth(n):
    return -(-int(n) // 1024) + 22


def dd_input(n_terms):
    return gamma(85) * float(n_terms)


def fresh_state(**kw):
    st = {"fine_freq_offset": 0.0, "coarse_freq_offset": 0.0, "signal_average": 0.0, "last_fine_error": 0.0,
          "total_frames_read": 0, "total_frames_desync": 0, "tracking": 0, "last_time_offset": 0, "next_frame_start": 0.0,
          "drift": 0.0, "last_peak_to_mean": 0.0, "loop_gated": 0, "dd_branch": 0, "dd_pending": 0}
    st.update(kw)
    return st


def state_of(rec):
    """A numpy STREAM_STATE record (or a dict) as a plain dict of Python numbers."""
    names = rec.dtype.names if hasattr(rec, "dtype") else rec.keys()
    return {k: (float(rec[k]) if isinstance(fresh_state()[k], float) else int(rec[k])) for k in names if k in fresh_state()}


def _options(value, ambiguous):
    return [value, not value] if ambiguous else [value]


def _rint_options(v, dv):
    """Integers rint(v) may give when v carries an error of dv."""
    lo, hi = math.floor(v - dv + 0.5), math.floor(v + dv + 0.5)
    k0 = int(np.rint(v))
    return sorted({k0, int(lo), int(hi)}, key=lambda k: (k != k0, k))


def angle_mean(z, q):
    """(sum of angle(z)) / q and its budget."""
    th = np.angle(np.asarray(z).astype(np.complex128)).ravel()
    m = float(th.sum()) / q
    return m, (C_ATAN2 * U + gamma(depth(th.size))) * float(np.abs(th).sum()) / q + U * abs(m)


def cp_error(rows):
    """err of the cyclic-prefix loop over rows [frames][76] -> (err, derr)."""
    rows = np.asarray(rows)
    m, dm = angle_mean(rows, rows.size)
    e = m * K_CP
    return e, dm * K_CP + 2 * U * abs(e)


def level_of(samples):
    x = np.asarray(samples).astype(np.complex128).ravel()[:LEVEL_SAMPLES]
    assert x.size == LEVEL_SAMPLES
    lv = float((np.abs(x.real) + np.abs(x.imag)).sum()) / LEVEL_SAMPLES
    return lv, (gamma(32) + U) * lv


def dd_errors(state, rows, gate, terms_per_frame=TERMS_PER_FRAME, ds_input=0.0):
    """The decision-directed estimate of a call -> list of dicts (err, derr, loop_gated, dd_branch, dd_pending, gated, k_raw),
    the reference's own outcome first."""
    a = np.asarray(rows).astype(np.complex128).reshape(-1, NB_SYMBOLS)
    frames = a.shape[0]
    body = a[:, 1:]
    S = complex(body.sum())
    n_terms = float(frames) * float(terms_per_frame)
    dS = gamma(depth(body.size)) * float(np.abs(body.real).sum() + np.abs(body.imag).sum()) + ds_input
    m, dm = angle_mean(a[:, 0], frames)
    e_cp = m * K_CP
    de_cp = dm * K_CP + 2 * U * abs(e_cp)
    g = float(np.float32(gate))
    mag2, thr = abs(S) ** 2, g * g * n_terms
    dmag2 = 2 * abs(S) * dS + dS * dS + 3 * U * mag2 + 2 * U * thr
    gated0 = (not n_terms > 0.0) or mag2 < thr
    first = int(state["total_frames_read"]) == 0
    out = []
    for gated in _options(gated0, n_terms > 0.0 and abs(mag2 - thr) <= dmag2):
        if gated:
            v = e_cp / STEP
            for k in _rint_options(v, de_cp / STEP + 2 * U * abs(v)):
                out.append(dict(err=e_cp, derr=de_cp, loop_gated=int(state["loop_gated"]) + 1, dd_branch=k,
                                dd_pending=DD_NO_BRANCH, gated=True, k_raw=k))
            continue
        ang = math.atan2(-S.imag, -S.real)
        dang = math.asin(min(1.0, dS / abs(S))) + C_ATAN2 * U * abs(ang)
        e_dd = ang * K_DD
        de_dd = dang * K_DD + 2 * U * abs(e_dd)
        v = (e_cp - e_dd) / STEP
        for k_raw in _rint_options(v, (de_cp + de_dd) / STEP + 3 * U * abs(v)):
            k, lg, pend = k_raw, int(state["loop_gated"]), DD_NO_BRANCH
            if not first and int(state["dd_branch"]) == 0 and k in (1, -1) and int(state["dd_pending"]) != k:
                pend, lg, k = k, lg + 1, 0
            e = e_dd + k * STEP
            out.append(dict(err=e, derr=de_dd + U * abs(k) * STEP + U * abs(e), loop_gated=lg, dd_branch=k, dd_pending=pend,
                            gated=False, k_raw=k_raw))
    return out


def fine_loop(state, rows, level_samples, n_frames, beta, thr_null_start=0.35, signal_beta=0.95, dd=False, dd_gate=2.5,
              terms_per_frame=TERMS_PER_FRAME, ds_input=0.0):
    """Fine-frequency loop, level and gate memory of one call over the rows [n_frames][76] that count.  -> list of outcome
    dicts: the new values of fine_freq_offset, last_fine_error, signal_average, loop_gated, dd_branch, dd_pending, plus
    level_lost, steers, wrap_edge, and the budgets d_fine, d_err, d_level (relative)."""
    beta, thr, sb = float(np.float32(beta)), float(np.float32(thr_null_start)), float(np.float32(signal_beta))
    fine, avg = float(state["fine_freq_offset"]), float(state["signal_average"])
    lv, dlv = level_of(level_samples)
    lost0 = avg > 0.0 and lv < thr * avg
    out = []
    for lost in _options(lost0, avg > 0.0 and abs(lv - thr * avg) <= dlv + 2 * U * thr * avg):
        steers = not (lost and n_frames == 1)
        if dd:
            errs = dd_errors(state, rows, dd_gate, terms_per_frame, ds_input)
        else:
            e, de = cp_error(rows)
            errs = [dict(err=e, derr=de)]
        for e in errs:
            o = dict(level_lost=lost, steers=steers, last_fine_error=e["err"], d_err=e["derr"], wrap_edge=False,
                     fine_freq_offset=fine, d_fine=0.0, level=lv,
                     loop_gated=int(state["loop_gated"]), dd_branch=int(state["dd_branch"]), dd_pending=int(state["dd_pending"]))
            if steers:
                f = fine - beta * e["err"]
                df = beta * e["derr"] + U * abs(beta * e["err"]) + U * abs(f)
                o["wrap_edge"] = abs(abs(f) - HALF) <= df
                if f > HALF:
                    f -= 2 * HALF
                    df += U * abs(f)
                elif f < -HALF:
                    f += 2 * HALF
                    df += U * abs(f)
                o["fine_freq_offset"], o["d_fine"] = f, df
                if dd:
                    o.update(loop_gated=e["loop_gated"], dd_branch=e["dd_branch"], dd_pending=e["dd_pending"])
            if lost:
                o["signal_average"], o["d_level"] = avg, 0.0
            elif avg > 0.0:
                new = sb * avg + (1.0 - sb) * lv
                o["signal_average"], o["d_level"] = new, ((1.0 - sb) * dlv + 4 * U * new) / new
            else:
                o["signal_average"], o["d_level"] = lv, dlv / lv if lv > 0 else 0.0
            out.append(o)
    return out


def stream_update(state, rows, last_frame, beta, thr_null_start=0.35, signal_beta=0.95, dd=False, dd_gate=2.5,
                  terms_per_frame=TERMS_PER_FRAME, ds_input=0.0):
    """The stream call's state update for one stream.  rows: [frames][76]; last_frame: the stream's last frame from its
    first PRS sample (>= 4096 samples).  -> list of outcomes (whole new states plus the fine_loop extras)."""
    rows = np.asarray(rows).reshape(-1, NB_SYMBOLS)
    frames = rows.shape[0]
    out = []
    for o in fine_loop(state, rows, last_frame, frames, beta, thr_null_start, signal_beta, dd, dd_gate, terms_per_frame, ds_input):
        new = dict(state)
        new.update(o)
        if o["level_lost"]:
            new["total_frames_desync"] = int(state["total_frames_desync"]) + 1
            new["total_frames_read"] = int(state["total_frames_read"]) + frames - 1
        else:
            new["total_frames_read"] = int(state["total_frames_read"]) + frames
        out.append(new)
    return out


# ------------------------------------------------------------------------------------------------------ timing tracking
def predict(state, n_samples, max_frames):
    """-> (j0, [slot positions inside the capture], period).  Positions in extended precision before the rounding."""
    nxt, period = LD(float(state["next_frame_start"])), LD(L_FRAME) + LD(float(np.float32(state["drift"])))
    j0 = 0
    if nxt < 0:
        j0 = int(np.ceil(-nxt / period))
        while nxt + LD(j0) * period < 0:                          # (the quotient's rounding)
            j0 += 1
        while j0 > 0 and nxt + LD(j0 - 1) * period >= 0:
            j0 -= 1
    slots = []
    for i in range(max_frames):
        c = int(np.rint(nxt + LD(j0 + i) * period))
        if c < 0 or c + FRAME_LEN + FIT_SLACK > n_samples:
            break
        slots.append(c)
    return j0, slots, period


def position(state, j0, i):
    return LD(float(state["next_frame_start"])) + LD(j0 + i) * (LD(L_FRAME) + LD(float(np.float32(state["drift"]))))


def position_ties(state, j0, count, eps=1e-6):
    """Slots whose unrounded position lies within eps of a rounding tie (none in a well-made case)."""
    return [i for i in range(count + 1) if abs(abs(float(position(state, j0, i) % 1) - 0.5)) < eps]


def line(idx, res, dres, count_one):
    """Least-squares line through (idx, res) -> dict alpha, slope, slope_hat, gain factor, d_alpha, d_slope.  One point:
    alpha = res, slope 0, slope_hat = res when the call had one slot."""
    n = len(idx)
    i = np.asarray(idx, LD)
    r = np.asarray(res, LD)
    dr = np.asarray(dres, np.float64)
    if n == 0:
        return dict(alpha=0.0, slope=0.0, slope_hat=0.0, factor=0.0, d_alpha=0.0, d_slope=0.0, d_slope_hat=0.0)
    if n == 1:
        a = float(r[0])
        return dict(alpha=a, slope=0.0, slope_hat=a if count_one else 0.0, factor=0.125, d_alpha=float(dr[0]), d_slope=0.0,
                    d_slope_hat=float(dr[0]) if count_one else 0.0)
    si, sii, sr, sir = i.sum(), (i * i).sum(), r.sum(), (i * r).sum()
    det = LD(n) * sii - si * si
    slope = (LD(n) * sir - si * sr) / det
    alpha = (sr - slope * si) / LD(n)
    R = np.abs(np.asarray(res, np.float64)) + dr
    fi = np.asarray(idx, np.float64)
    d_slope = (gamma(n + 3, U64) * (n * float((fi * R).sum()) + float(fi.sum()) * float(R.sum())) + n * float((fi * dr).sum()) +
               float(fi.sum()) * float(dr.sum())) / float(det) + 3 * U64 * abs(float(slope))
    d_alpha = (gamma(n, U64) * float(R.sum()) + float(dr.sum()) + d_slope * float(si) + 2 * U64 * abs(float(slope * si))) / n + \
        2 * U64 * abs(float(alpha))
    return dict(alpha=float(alpha), slope=float(slope), slope_hat=float(slope), factor=min(1.0, n / 4.0), d_alpha=d_alpha,
                d_slope=d_slope, d_slope_hat=d_slope)


def track_update(state, frames, rows, level_samples, n_samples, max_frames, advance, fine_beta=0.9, drift_beta=0.5,
                 signal_beta=0.95, thr_null_start=0.35, dd=False, dd_gate=2.5, terms_per_frame=TERMS_PER_FRAME, ds_input=0.0,
                 fixed_start=False):
    """State after a tracked call for one stream.  frames: records with start, flags, peak_to_mean for the slots (at least
    count of them); rows: [slots][76] loop input (unlocked rows ignored); level_samples: 4096 samples from the last locked
    frame's start (None when nothing locked).  fixed_start: the frame call (one slot, no timing).
    -> (list of outcomes, count); an outcome is the whole new state plus budgets d_fine, d_err, d_level, d_next, d_drift."""
    if not fixed_start and int(state["tracking"]) != 1:
        return [dict(state)], 0
    if fixed_start:
        j0, count = 0, 1
    else:
        j0, slots, _ = predict(state, n_samples, max_frames)
        count = len(slots)
    locked = [i for i in range(count) if (int(frames[i]["flags"]) & 3) == 3]
    n = len(locked)
    rows = np.asarray(rows).reshape(-1, NB_SYMBOLS)
    if n:
        loops = fine_loop(state, rows[locked], level_samples, n, fine_beta, thr_null_start, signal_beta, dd, dd_gate,
                          terms_per_frame, ds_input)
    else:
        loops = [None]
    res = [LD(int(frames[i]["start"])) - position(state, j0, i) for i in locked]
    dres = [2 * U64 * abs(float(position(state, j0, i))) + U64 * abs(float(r)) for i, r in zip(locked, res)]
    ln = line(locked, res, dres, count == 1)
    gain = float(np.float32(drift_beta)) * ln["factor"]
    out = []
    for o in loops:
        new = dict(state)
        new.update(d_fine=0.0, d_err=0.0, d_level=0.0, d_next=0.0, d_drift=0.0, level_lost=False, wrap_edge=False)
        lost = False
        if o is not None:
            new.update(o)
            lost = o["level_lost"]
            last = locked[-1]
            if not fixed_start:
                new["last_time_offset"] = int(frames[last]["start"]) - int(np.rint(position(state, j0, last)))
            new["last_peak_to_mean"] = float(frames[last]["peak_to_mean"])
        if not fixed_start:
            if count > 0 and n == 0:
                new["tracking"] = 0
            pc = position(state, j0, count)
            nxt = pc + LD(ln["alpha"]) + LD(ln["slope"]) * LD(count) - LD(int(advance))
            new["next_frame_start"] = float(nxt)
            new["d_next"] = ln["d_alpha"] + count * ln["d_slope"] + 4 * U64 * max(abs(float(pc)), abs(float(advance)), abs(float(nxt)))
            drift = float(np.float32(state["drift"])) + gain * ln["slope_hat"]
            new["drift"] = drift
            new["d_drift"] = gain * ln["d_slope_hat"] + U * abs(drift)
        new["total_frames_read"] = int(state["total_frames_read"]) + n - (1 if lost else 0)
        new["total_frames_desync"] = int(state["total_frames_desync"]) + j0 + (count - n) + (1 if lost else 0)
        new["alpha"], new["slope"], new["d_alpha"], new["d_slope"] = ln["alpha"], ln["slope"], ln["d_alpha"], ln["d_slope"]
        out.append(new)
    return out, count


def coarse_update(coarse, k_hat, locked, acquiring, max_coarse, slow_beta=0.1):
    """The frame call's coarse offset after the PRS search -> (coarse, budget)."""
    coarse = float(np.float32(coarse))
    if max_coarse <= 0 or not locked:
        return coarse, 0.0
    if acquiring:
        return -float(k_hat) / NB_FFT, 0.0
    if k_hat == 0:
        return coarse, 0.0
    new = coarse - float(np.float32(slow_beta)) * float(k_hat) / NB_FFT
    return new, 2 * U * abs(new) + 2 * U * abs(float(np.float32(slow_beta)) * float(k_hat) / NB_FFT)


def track_start(state, frames, count, max_frames, advance, only_lost=False):
    """State after dabgpu_track_start_dev for one stream.  frames: acquisition records (start, flags, fine_offset,
    coarse_carriers, peak_to_mean).  -> the new state plus budgets d_drift, d_next, d_fine (one outcome: nothing is
    ambiguous here but a frame-number tie, which raises)."""
    new = dict(state)
    new.update(d_drift=0.0, d_next=0.0, d_fine=0.0)
    if only_lost and int(state["tracking"]) == 1:
        return new
    count = min(int(count), int(max_frames))
    locked = [i for i in range(count) if (int(frames[i]["flags"]) & 3) == 3]
    if not locked:
        new["tracking"] = 0
        return new
    n = len(locked)
    s0 = int(frames[locked[0]]["start"])
    y = [int(frames[i]["start"]) - s0 for i in locked]
    for v in y:
        assert abs(abs(Fraction(v, L_FRAME) % 1 - Fraction(1, 2))) > Fraction(1, 1000), "frame-number tie"
    j = [int(math.floor(Fraction(v, L_FRAME) + Fraction(1, 2))) for v in y]
    drift = 0.0
    if n >= 4:
        sj, sjj, sy, sjy = sum(j), sum(a * a for a in j), sum(y), sum(a * b for a, b in zip(j, y))
        drift = float(Fraction(n * sjy - sj * sy, n * sjj - sj * sj) - L_FRAME)
        new["d_drift"] = 4 * U64 * L_FRAME + U * abs(drift)
    last = locked[-1]
    new["drift"] = drift
    new["next_frame_start"] = float(int(frames[last]["start"]) + L_FRAME - int(advance)) + drift
    new["d_next"] = new["d_drift"] + 4 * U64 * abs(float(int(frames[last]["start"])))
    f = [float(np.float32(frames[i]["fine_offset"])) for i in locked]
    new["fine_freq_offset"] = math.fsum(f) / n
    new["d_fine"] = (gamma(depth(n)) + U) * math.fsum(abs(v) for v in f) / n
    new["coarse_freq_offset"] = -float(int(frames[last]["coarse_carriers"])) / NB_FFT
    new["tracking"] = 2 if only_lost else 1
    new["dd_branch"] = new["dd_pending"] = DD_NO_BRANCH
    new["total_frames_read"] = int(state["total_frames_read"]) + n
    new["last_time_offset"] = 0
    new["last_peak_to_mean"] = float(frames[last]["peak_to_mean"])
    return new


# ------------------------------------------------------------------------------------------------------ acceptance
INT_FIELDS = ("total_frames_read", "total_frames_desync", "tracking", "last_time_offset", "loop_gated", "dd_branch", "dd_pending")


def mod_carrier(d):
    return (d + HALF) % (2 * HALF) - HALF


def compare(got, want, fields=None):
    """got: a state (dict / record) against ONE outcome -> (None, fractions of budgets used) or (what differs, None)."""
    frac = {}
    for k in INT_FIELDS:
        if (fields is None or k in fields) and k in want and int(got[k]) != int(want[k]):
            return "%s: %d, reference %d" % (k, int(got[k]), int(want[k])), None

    def near(k, budget, what, mod=False):
        d = float(got[k]) - float(want[k])
        if mod:
            d = mod_carrier(d)
        if abs(d) > budget:
            return "%s: %.12g, reference %.12g, off by %.3g, budget %.3g" % (k, float(got[k]), float(want[k]), d, budget)
        if budget > 0:
            frac[what] = max(frac.get(what, 0.0), abs(d) / budget)
        return None

    checks = [("fine_freq_offset", want.get("d_fine", 0.0), "fine", bool(want.get("wrap_edge"))),
              ("last_fine_error", want.get("d_err", 0.0), "err", False),
              ("signal_average", want.get("d_level", 0.0) * abs(float(want["signal_average"])), "level", False),
              ("next_frame_start", want.get("d_next", 0.0), "next", False),
              ("drift", want.get("d_drift", 0.0), "drift", False),
              ("coarse_freq_offset", want.get("d_coarse", 0.0), "coarse", False),
              ("last_peak_to_mean", 0.0, "ptm", False)]
    for k, b, what, mod in checks:
        if fields is not None and k not in fields:
            continue
        bad = near(k, b, what, mod)
        if bad:
            return bad, None
    return None, frac


def accept(got, outcomes, fields=None):
    """got against the outcome list: passes when ANY outcome matches (one outcome when the case is unambiguous).
    -> fractions of budgets used; raises AssertionError with every outcome's first difference otherwise."""
    why = []
    for o in outcomes:
        bad, frac = compare(got, o, fields)
        if bad is None:
            return frac
        why.append(bad)
    raise AssertionError("no reference outcome matches: " + " | ".join(why))


def budgets_within_bars(o):
    """The derived budgets of an outcome against the bars test_tracking.check_state uses -> list of violations."""
    bad = []
    if o.get("d_fine", 0.0) > BAR_FINE:
        bad.append(("d_fine", o["d_fine"]))
    if o.get("d_err", 0.0) > BAR_FINE:
        bad.append(("d_err", o["d_err"]))
    if o.get("d_next", 0.0) > BAR_NEXT:
        bad.append(("d_next", o["d_next"]))
    if o.get("d_drift", 0.0) > BAR_REL + BAR_REL * abs(float(o.get("drift", 0.0))):
        bad.append(("d_drift", o["d_drift"]))
    if o.get("d_level", 0.0) > BAR_REL:
        bad.append(("d_level", o["d_level"]))
    return bad
