"""The OFDM front end (rows A2..A6) against the float64 from-definition reference tests/ofdm_reference.py.

Bars, per soft bit (v = the reference's soft value, eps its band, both derived in the reference's docstring):
- where v is farther than eps from a point where trunc jumps, the kernel's bit is trunc(v) EXACTLY; inside, within 1 LSB;
- the larger component of every carrier with d != 0 is exactly +-127; d == 0 gives (0, 0);
- the share of bits inside the band is reported and, at 8 dB SNR and above, held under BAND_MAX (else the bar is vacuous).
Spectra, constellation, cyclic-prefix correlations and dd4 sums: each element within its own budget (not a fraction of
a peak).  The CPU tests check the reference itself: its tables, its signs against the transmitted bits, its FFT against a
direct DFT, and its bands against the float32 oracle (exact outside the band)."""
import numpy as np
import pytest

import ofdm_reference as R
from dabgpu import synth

BAND_MAX = 0.02

FRAME = R.FRAME_SAMPLES
TIE_UP = float(np.float32(3 * 2.0 ** -33))                 # f 2^32 = 1.5 -> dphi 2 (ties to even: up)
TIE_DOWN = float(np.float32(-(2 ** 23 + 1) * 2.0 ** -33))  # f 2^32 = -(2^22 + 0.5) -> -2^22 (ties to even: down)
CORRECTIONS = [0.0, 2.0 ** -32, -2.0 ** -32, 0.37 / 2048, -0.37 / 2048, 5.2 / 2048, -5.2 / 2048, 200 / 2048, -200 / 2048,
               0.5, -0.5, TIE_UP, TIE_DOWN]
# two of test_gpu_parity.py's realistic channels: three echoes inside the prefix; a late echo stronger than the first
# path (deep spectral notches)
CHANNELS = {
    "three_taps": dict(snr_db=22.0, paths=[(0, 1.0), (37, 0.5 * np.exp(1.0j)), (180, 0.35 * np.exp(-2.0j))]),
    "late_echo_2dB_stronger": dict(snr_db=24.0, paths=[(0, 1.0), (250, 1.26 * np.exp(0.4j))]),
}


# ------------------------------------------------------------------------------------------------------------- inputs
def open_loop_frames(ensemble_iq, snr):
    """One frame per correction f (frame i: transmitted frame i % 5 shifted by -f, so that the correction undoes it)
    -> (frames [13][76*2552] complex64, f [13] float32)."""
    fo = np.array(CORRECTIONS, np.float32)
    out = []
    for i, f in enumerate(fo):
        rng = np.random.default_rng(100 + i + (0 if snr is None else int(snr)))
        x = synth.channel(ensemble_iq[i % ensemble_iq.shape[0]], snr_db=snr, cfo=-float(f), rng=rng)
        out.append(x[synth.NB_NULL:synth.NB_NULL + FRAME])
    return np.ascontiguousarray(np.stack(out)), fo


def channel_frames(ensemble_iq, name, n_frames=4):
    """Frames of a stream through CHANNELS[name] with a residual 0.23 carriers, FFT windows 32 samples early."""
    kw = dict(CHANNELS[name])
    rng = np.random.default_rng(sum(map(ord, name)))
    cfo = 0.23 / 2048
    rx = synth.channel(ensemble_iq[:n_frames + 1].ravel(), cfo=cfo, rng=rng, **kw)
    starts = [f * synth.NB_FRAME_SAMPLES + synth.NB_NULL - 32 for f in range(n_frames)]
    return np.ascontiguousarray(np.stack([rx[s:s + FRAME] for s in starts])), np.full(n_frames, -cfo, np.float32)


def quantise(x, fmt):
    """complex samples -> (integer array [..., 2] of format fmt, complex128 values the reference is fed)."""
    v = np.stack([x.real, x.imag], axis=-1).astype(np.float64)
    v *= {"cs16": 2000.0, "cs8": 25.0, "cu8": 25.0}[fmt] / np.sqrt(np.mean(v * v))
    if fmt == "cs16":
        q = np.clip(np.rint(v), -32768, 32767).astype(np.int16)
        val = q.astype(np.float64)
    elif fmt == "cs8":
        q = np.clip(np.rint(v), -128, 127).astype(np.int8)
        val = q.astype(np.float64)
    else:
        q = np.clip(np.rint(v + 127.5), 0, 255).astype(np.uint8)
        val = R.cu8_values(q)
    return q, val[..., 0] + 1j * val[..., 1]


# ------------------------------------------------------------------------------------------------------------- the bars
def check_soft(got, fr, label, snr=None, rows=None):
    """Hold soft bits [230400] (or the data-symbol rows `rows` of them) to the reference frame fr; returns the share of
    bits inside the band (the larger components, pinned exactly, are not counted)."""
    shape = (R.NB_DATA_SYMBOLS, 2, R.NB_CARRIERS)
    sel = slice(None) if rows is None else rows
    got = np.asarray(got, np.int8).reshape(shape)[sel].astype(np.int32)
    want = fr.soft().reshape(shape)[sel].astype(np.int32)
    v, eps = fr.v.reshape(shape)[sel], fr.eps.reshape(shape)[sel]
    band = fr.in_band().reshape(shape)[sel]
    larger = fr.larger_component().reshape(shape)[sel]
    erased = fr.erased()[sel]
    # erasures
    assert not got[np.repeat(erased[:, None, :], 2, axis=1)].any(), "%s: d == 0 must give (0, 0)" % label
    # the larger component is exactly +-127, whatever the band says
    live = ~erased
    assert (np.maximum(np.abs(got[:, 0]), np.abs(got[:, 1]))[live] == 127).all(), "%s: larger component != 127" % label
    assert (got[larger] == want[larger]).all(), "%s: larger component has the wrong sign or place" % label
    # outside the band: exact; inside: 1 LSB
    bad = ~band & (got != want)
    assert not bad.any(), "%s: %d soft bits outside the band differ from trunc(v) (first: got %d, v = %.6f, eps %.2e)" % (
        label, bad.sum(), got[bad][0], v[bad][0], eps[bad][0])
    assert np.abs(got - want).max(initial=0) <= 1, label
    frac = float((band & ~larger & live[:, None, :]).mean())
    print("band %-48s %.4f" % (label, frac))
    if snr is not None and snr >= 8.0:
        assert frac < BAND_MAX, "%s: %.4f of the bits inside the band" % (label, frac)
    return frac


def check_within(got, want, budget, label):
    err = np.abs(np.asarray(got, np.complex128) - want)
    budget = np.broadcast_to(budget, err.shape)
    assert not err[budget == 0].any(), "%s: an element whose budget is 0 is not exact" % label
    ratio = float((err[budget > 0] / budget[budget > 0]).max(initial=0.0))
    assert ratio <= 1.0, "%s: error %.3g of its budget" % (label, ratio)
    return ratio


def check_cyc(got, fr, label):
    check_within(got, fr.cyc, fr.cyc_budget, label + " cyc")


# ------------------------------------------------------------------------------------------------------------- CPU
def test_deinterleaver_is_a_permutation_with_known_answer():
    car = R.CARRIERS
    assert car.size == 1536 and sorted(car.tolist()) == sorted(set(range(-768, 769)) - {0})
    # the known-answer entries of test_tables.py (PI = 0, 511, 1010, 1353, 1716, 291, 1037 ...)
    assert car[:6].tolist() == [-513, -14, 329, 692, -733, 13]
    assert sorted(R.DATA_BINS.tolist()) == sorted(R.ORDER_BINS.tolist())
    assert 0 not in R.DATA_BINS and 1024 not in R.DATA_BINS
    assert sorted(R.DD_BINS.tolist()) == sorted(set(range(1, 129)) - {128} | {768} | set(range(1920, 2048)))


def test_phase_step_quantisation():
    assert R.dphi_of(0.0) == 0 and R.dphi_of(2.0 ** -32) == 1 and R.dphi_of(-2.0 ** -32) == (1 << 32) - 1
    assert R.dphi_of(0.5) == R.dphi_of(-0.5) == 1 << 31
    assert R.dphi_of(TIE_UP) == 2 and R.dphi_of(TIE_DOWN) == (1 << 32) - (1 << 22)
    # the phase is exact integer arithmetic: dphi = 2^31 alternates +1, -1
    assert np.allclose(R.nco(6, 1 << 31), [1, -1, 1, -1, 1, -1], atol=1e-15)
    assert R.stream_correction(0.1 / 2048, -3 / 2048) == np.float32(np.float32(0.1 / 2048) + np.float32(-3 / 2048))


def test_noise_free_signs_are_the_transmitted_bits(ensemble, ensemble_iq):
    frames, fo = open_loop_frames(ensemble_iq, None)
    for i in (0, 5, 7, 9):
        fr = R.Frame(frames[i], fo[i])
        bits = ensemble.frame_bits[i % ensemble.n_frames].astype(bool)
        assert ((fr.v > 0) == bits).all(), i
        assert (np.abs(fr.v) > 126.99).all()


def test_fft_stage_matches_a_direct_dft(ensemble_iq):
    frames, fo = open_loop_frames(ensemble_iq, 8.0)
    n = np.arange(R.NB_FFT)
    W = np.exp(-2j * np.pi * np.outer(n, n) / R.NB_FFT)
    for i, l in ((3, 0), (7, 37), (9, 75)):
        fr = R.Frame(frames[i], fo[i])
        y = frames[i].astype(np.complex128) * R.nco(FRAME, R.dphi_of(fo[i]))
        direct = W @ y[l * R.NB_SYM + R.NB_CP:(l + 1) * R.NB_SYM]
        assert np.abs(fr.X[l] - direct).max() <= 1e-9 * np.abs(direct).max()
        assert np.abs(fr.X[l] - direct).max() < 1e-3 * fr.E[l]         # the reference's own error is far below the budget


def _oracle_cases(ensemble_iq):
    for snr in (8.0, 20.0):
        frames, fo = open_loop_frames(ensemble_iq, snr)
        for i in range(len(fo)):
            yield "snr%g f%d" % (snr, i), frames[i], fo[i]
    for name in sorted(CHANNELS):
        frames, fo = channel_frames(ensemble_iq, name, 2)
        for i in range(len(fo)):
            yield "%s f%d" % (name, i), frames[i], fo[i]


def test_reference_band_holds_the_float32_oracle(built, ensemble_iq):
    """The oracle (float32, radix-2, double-precision NCO) is a correct float32 implementation: outside the reference's
    band its soft bits are trunc(v) exactly, inside within 1 LSB; its spectra and correlations stay within budget; and
    the band is narrow (not vacuous)."""
    from oracle import oracle as O
    for label, x, f in _oracle_cases(ensemble_iq):
        fr = R.Frame(x, f)
        osoft, ospec, ocyc, odq = O.ofdm_demod_frame(x, float(f), want_spectra=True, want_cyc=True, want_dqpsk=True)
        v = fr.soft().astype(np.int32)
        band = fr.in_band()
        d = osoft.astype(np.int32) - v
        assert not d[~band].any(), label
        assert np.abs(d).max() <= 1, label
        frac = float((band & ~fr.larger_component()).mean())
        assert frac < BAND_MAX, (label, frac)
        check_within(ospec, fr.X, fr.E[:, None], label + " spectra")
        check_cyc(ocyc, fr, label)
        dq, b = fr.dqpsk()
        check_within(odq, dq, b, label + " dqpsk")


def test_reference_dd4_matches_the_oracle(built, ensemble_iq):
    from oracle import oracle as O
    frames, fo = open_loop_frames(ensemble_iq, 12.0)
    for i in (0, 4, 8):
        fr = R.Frame(frames[i], fo[i])
        _, dd4 = O.ofdm_demod_frame_dd(frames[i], float(fo[i]))
        t, b = fr.dd4_terms()
        _, bud = R.dd4_expected(fr, 1)
        assert abs(complex(dd4[1:].astype(np.complex128).sum()) - t[1:].sum()) <= bud[75], i
        assert abs(complex(dd4[0]) - t[0]) <= b[0], i


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("snr", [None, 8.0, 20.0], ids=["noise_free", "8dB", "20dB"])
def test_gpu_open_loop_host_and_dev(gctx, ensemble_iq, snr):
    torch, dev = _torch()
    frames, fo = open_loop_frames(ensemble_iq, snr)
    n = len(fo)
    soft, cyc, dq = gctx.ofdm_demod_frames(frames, fo, want_cyc=True, want_dqpsk=True)
    d_iq = torch.from_numpy(frames).to(dev)
    d_fo = torch.from_numpy(fo).to(dev)
    d_soft = torch.zeros((n, R.NB_FRAME_BITS), dtype=torch.int8, device=dev)
    d_cyc = torch.zeros((n, 76), dtype=torch.complex64, device=dev)
    gctx.ofdm_demod_frames_dev(d_iq.data_ptr(), FRAME, n, d_fo.data_ptr(), d_soft.data_ptr(), d_cyc.data_ptr())
    gctx.sync()
    assert (d_soft.cpu().numpy() == soft).all() and (d_cyc.cpu().numpy() == cyc).all()
    for i in range(n):
        fr = R.Frame(frames[i], fo[i])
        label = "open loop %s f=%.6g" % ("none" if snr is None else "%gdB" % snr, fo[i] * 2048)
        check_soft(soft[i], fr, label, snr)
        check_cyc(cyc[i], fr, label)
        want, budget = fr.dqpsk()
        check_within(dq[i], want, budget, label + " dqpsk")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CHANNELS))
def test_gpu_open_loop_through_channels(gctx, ensemble_iq, name):
    frames, fo = channel_frames(ensemble_iq, name)
    soft, cyc, dq = gctx.ofdm_demod_frames(frames, fo, want_cyc=True, want_dqpsk=True)
    for i in range(len(fo)):
        fr = R.Frame(frames[i], fo[i])
        check_soft(soft[i], fr, "%s frame %d" % (name, i), CHANNELS[name]["snr_db"])
        check_cyc(cyc[i], fr, name)
        want, budget = fr.dqpsk()
        check_within(dq[i], want, budget, name + " dqpsk")


@pytest.mark.gpu
def test_gpu_fft_symbols_at_every_correction(gctx, ensemble_iq):
    frames, fo = open_loop_frames(ensemble_iq, 20.0)
    spec = gctx.fft_symbols(frames, fo)
    worst = 0.0
    for i in range(len(fo)):
        fr = R.Frame(frames[i], fo[i])
        worst = max(worst, check_within(spec[i], fr.X, fr.E[:, None], "fft_symbols f=%g" % (fo[i] * 2048)))
    spec0 = gctx.fft_symbols(frames[:1])                                  # the kernel without the NCO
    fr = R.Frame(frames[0], 0.0)
    check_within(spec0[0], fr.X, fr.E[:, None], "fft_symbols, no correction")
    print("fft_symbols: worst error / budget %.3f" % worst)


def _acquired_case(fmt, starts, fos, base, total):
    """Frames at `starts` of one stream of `total` samples (format fmt), allocated on the device and written only where
    the frames are -> soft, cyc of ofdm_demod_acquired_dev, the reference frames."""
    import dabgpu
    torch, dev = _torch()
    n = len(starts)
    rng = np.random.default_rng(77)
    refs, vals = [], []
    for i, (s, f) in enumerate(zip(starts, fos)):
        x = synth.channel(base[i % base.shape[0]], snr_db=12.0, cfo=-float(f), rng=rng)[synth.NB_NULL:synth.NB_NULL + FRAME]
        if fmt == "cf32":
            q, val = x, x.astype(np.complex128)
        else:
            q, val = quantise(x, fmt)
        vals.append(q)
        refs.append(R.Frame(val, np.float32(f)))
    elem = {"cf32": (torch.float32, 2), "cs16": (torch.int16, 2), "cs8": (torch.int8, 2), "cu8": (torch.uint8, 2)}[fmt]
    buf = torch.empty(total * elem[1], dtype=elem[0], device=dev)
    try:
        for s, q in zip(starts, vals):
            flat = np.ascontiguousarray(q).view(np.float32).reshape(-1) if fmt == "cf32" else np.ascontiguousarray(q).reshape(-1)
            buf[2 * s:2 * s + flat.size].copy_(torch.from_numpy(flat).to(dev))
        rec = np.zeros(n, dabgpu.ACQUIRED_FRAME_DTYPE)
        rec["start"] = starts
        rec["freq_offset"] = fos
        rec["flags"] = 3
        d_rec = torch.from_numpy(rec.view(np.uint8)).to(dev)
        soft = torch.zeros((n, R.NB_FRAME_BITS), dtype=torch.int8, device=dev)
        cyc = torch.zeros((n, 76), dtype=torch.complex64, device=dev)
        torch.cuda.synchronize()
        return (buf, d_rec, soft, cyc), refs
    except BaseException:
        del buf
        torch.cuda.empty_cache()
        raise


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,big", [("cf32", (1 << 29) + 12345), ("cs8", (1 << 31) + 7)],
                         ids=["cf32_byte_offset_above_2^32", "cs8_sample_index_above_2^31"])
def test_gpu_acquired_frames(gctx, ensemble_iq, fmt, big):
    import dabgpu
    torch, dev = _torch()
    starts = [1001, 200000, big, big + FRAME + 2]          # odd, even, far, far + even step
    fos = np.array([0.37 / 2048, -5.2 / 2048, 200 / 2048, -0.5], np.float32)
    total = big + 2 * FRAME + 64
    assert starts[2] * 8 > 1 << 32 if fmt == "cf32" else starts[2] > 1 << 31
    (buf, d_rec, soft, cyc), refs = _acquired_case(fmt, starts, fos, ensemble_iq, total)
    if fmt != "cf32":
        gctx.set_iq_format({"cs16": dabgpu.IQ_CS16, "cs8": dabgpu.IQ_CS8, "cu8": dabgpu.IQ_CU8}[fmt])
    try:
        gctx.ofdm_demod_acquired_dev(buf.data_ptr(), total, 1, len(starts), d_rec.data_ptr(), soft.data_ptr(),
                                     d_cyc=cyc.data_ptr())
        gctx.sync()
        got, gcyc = soft.cpu().numpy(), cyc.cpu().numpy()
    finally:
        gctx.set_iq_format(dabgpu.IQ_CF32)
        del buf
        torch.cuda.empty_cache()
    for i, fr in enumerate(refs):
        label = "acquired %s start %d" % (fmt, starts[i])
        check_soft(got[i], fr, label, 12.0)
        check_cyc(gcyc[i], fr, label)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["cs16", "cs8", "cu8"])
def test_gpu_integer_formats(gctx, ensemble_iq, fmt):
    """Integer samples against the reference fed the same integer values (cu8: u - 127.5), with and without the NCO, at
    an even and an odd frame stride."""
    import dabgpu
    torch, dev = _torch()
    frames, fo = open_loop_frames(ensemble_iq, 12.0)
    idx = [0, 3, 6, 8, 10]
    q, val = quantise(frames[idx], fmt)
    n = len(idx)
    gctx.set_iq_format({"cs16": dabgpu.IQ_CS16, "cs8": dabgpu.IQ_CS8, "cu8": dabgpu.IQ_CU8}[fmt])
    try:
        for stride in (FRAME, FRAME + 1):
            lay = np.zeros((n, stride, 2), q.dtype)
            lay[:, :FRAME] = q
            d_q = torch.from_numpy(lay).to(dev)
            d_fo = torch.from_numpy(np.ascontiguousarray(fo[idx])).to(dev)
            for with_nco in (True, False):
                soft = torch.zeros((n, R.NB_FRAME_BITS), dtype=torch.int8, device=dev)
                cyc = torch.zeros((n, 76), dtype=torch.complex64, device=dev)
                gctx.ofdm_demod_frames_dev(d_q.data_ptr(), stride, n, d_fo.data_ptr() if with_nco else None,
                                           soft.data_ptr(), cyc.data_ptr())
                gctx.sync()
                s, c = soft.cpu().numpy(), cyc.cpu().numpy()
                for k in range(n):
                    f = fo[idx[k]] if with_nco else 0.0
                    fr = R.Frame(val[k], f)
                    label = "%s stride %d nco %d f=%g" % (fmt, stride, with_nco, f * 2048)
                    check_soft(s[k], fr, label, 12.0 if (with_nco or f == 0) else None)
                    check_cyc(c[k], fr, label)
    finally:
        gctx.set_iq_format(dabgpu.IQ_CF32)


@pytest.mark.gpu
def test_gpu_closed_loop_streams(gctx, ensemble_iq):
    """ofdm_demod_streams(_dev): each call is held to the reference at the correction the stream states hold before the
    call (fine + coarse, added in float32 as the kernel adds them)."""
    torch, dev = _torch()
    S, F = 2, 2
    offsets = [(0.21 / 2048, -3.0 / 2048), (-0.33 / 2048, 7.0 / 2048)]
    rng = np.random.default_rng(31)
    iq = []
    for s in range(S):
        true_cfo = -(offsets[s][0] + offsets[s][1]) + 0.05 / 2048      # the loop has a residual to chase
        x = synth.channel(ensemble_iq[:F + 1].ravel(), snr_db=14.0, cfo=true_cfo, rng=rng)
        iq += [x[f * synth.NB_FRAME_SAMPLES + synth.NB_NULL:][:FRAME] for f in range(F)]
    iq = np.ascontiguousarray(np.stack(iq))
    for use_dev in (False, True):
        gctx.streams_reset(S)
        for s in range(S):
            gctx.set_stream_offsets(s, fine=offsets[s][0], coarse=offsets[s][1])
        for call in range(2):
            st = gctx.stream_states_host(S)
            if use_dev:
                d_iq = torch.from_numpy(iq).to(dev)
                soft_t = torch.zeros((S * F, R.NB_FRAME_BITS), dtype=torch.int8, device=dev)
                cyc_t = torch.zeros((S * F, 76), dtype=torch.complex64, device=dev)
                gctx.ofdm_demod_streams_dev(d_iq.data_ptr(), FRAME, S, F, 0.9, soft_t.data_ptr(), cyc_t.data_ptr())
                gctx.sync()
                soft, cyc = soft_t.cpu().numpy(), cyc_t.cpu().numpy()
            else:
                soft, cyc = gctx.ofdm_demod_streams(iq, S, want_cyc=True)
            for s in range(S):
                f = R.stream_correction(st["fine_freq_offset"][s], st["coarse_freq_offset"][s])
                for k in range(F):
                    fr = R.Frame(iq[s * F + k], f)
                    label = "streams%s call %d stream %d frame %d" % ("_dev" if use_dev else "", call, s, k)
                    check_soft(soft[s * F + k], fr, label, 14.0)
                    check_cyc(cyc[s * F + k], fr, label)
        after = gctx.stream_states_host(S)
        assert (after["fine_freq_offset"] != st["fine_freq_offset"]).any()         # the loop did move between calls


def _dd_case(ensemble_iq, runs):
    from conftest import make_ctx
    torch, dev = _torch()
    frames, fo = open_loop_frames(ensemble_iq, 12.0)
    idx = [0, 3, 5, 7, 11]
    n = len(idx)
    d_iq = torch.from_numpy(np.ascontiguousarray(frames[idx])).to(dev)
    d_fo = torch.from_numpy(np.ascontiguousarray(fo[idx])).to(dev)
    soft = torch.zeros((n, R.NB_FRAME_BITS), dtype=torch.int8, device=dev)
    dd4 = torch.zeros((n, 76), dtype=torch.complex64, device=dev)
    c = make_ctx(ofdm_symbol_runs=runs)
    try:
        c.ofdm_demod_frames_dd_dev(d_iq.data_ptr(), FRAME, n, d_fo.data_ptr(), soft.data_ptr(), dd4.data_ptr())
        c.sync()
    finally:
        c.close()
    return frames[idx], fo[idx], soft.cpu().numpy(), dd4.cpu().numpy().astype(np.complex128)


@pytest.mark.gpu
@pytest.mark.parametrize("runs", [1, 2, 75])
def test_gpu_decision_directed_sums(built, ensemble_iq, runs):
    frames, fo, soft, dd4 = _dd_case(ensemble_iq, runs)
    for i in range(len(fo)):
        fr = R.Frame(frames[i], fo[i])
        label = "dd runs %d frame %d" % (runs, i)
        check_soft(soft[i], fr, label, 12.0)
        want, budget = R.dd4_expected(fr, runs)
        zero = budget == 0
        assert (dd4[i][zero] == 0).all(), label + ": entries that are not a run's last symbol must be 0"
        check_within(dd4[i][~zero], want[~zero], budget[~zero], label + " dd4 per run")
        t, b = fr.dd4_terms()
        total_budget = budget[1:].sum()
        assert abs(dd4[i][1:].sum() - t[1:].sum()) <= total_budget, label + " dd4 frame sum"


@pytest.mark.gpu
@pytest.mark.parametrize("runs", [1, 2, 75])
def test_gpu_symbol_runs(built, ensemble_iq, runs):
    import dabgpu
    frames, fo = open_loop_frames(ensemble_iq, 8.0)
    idx = [1, 4, 7, 9]
    with dabgpu.Context(device=0, ofdm_symbol_runs=runs) as c:
        soft, cyc, _ = c.ofdm_demod_frames(frames[idx], fo[idx], want_cyc=True)
    for k, i in enumerate(idx):
        fr = R.Frame(frames[i], fo[i])
        check_soft(soft[k], fr, "runs %d frame %d" % (runs, i), 8.0)
        check_cyc(cyc[k], fr, "runs %d" % runs)


@pytest.mark.gpu
def test_gpu_large_batch_run_plan(built, ensemble_iq):
    """3072 + 45 frames: whole frames first, the rest cut (plan_runs); frames on both sides of the seam and the last."""
    import dabgpu
    torch, dev = _torch()
    frames, fo = open_loop_frames(ensemble_iq, 14.0)
    base_idx = [3, 5, 7, 12, 9]                 # corrections 0.37/2048, 5.2/2048, 200/2048, TIE_DOWN, 0.5
    k = len(base_idx)
    n = 3072 + 45
    base = torch.from_numpy(np.ascontiguousarray(frames[base_idx])).to(dev)
    iq = base.repeat((n + k - 1) // k, 1)[:n].contiguous()
    fo_all = torch.from_numpy(np.tile(fo[base_idx], (n + k - 1) // k)[:n].copy()).to(dev)
    try:
        with dabgpu.Context(device=0, max_frames=n) as c:
            soft = torch.zeros((n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
            cyc = torch.zeros((n, 76), dtype=torch.complex64, device=dev)
            torch.cuda.synchronize()
            c.ofdm_demod_frames_dev(iq.data_ptr(), iq.shape[1], n, fo_all.data_ptr(), soft.data_ptr(), cyc.data_ptr())
            c.sync()
            picked = {f: (soft[f].cpu().numpy(), cyc[f].cpu().numpy()) for f in (0, 3071, 3072, n - 1)}
    finally:
        del iq
        torch.cuda.empty_cache()
    for f, (s, cy) in picked.items():
        fr = R.Frame(frames[base_idx[f % k]], fo[base_idx[f % k]])
        check_soft(s, fr, "large batch frame %d" % f, 14.0)
        check_cyc(cy, fr, "large batch frame %d" % f)


@pytest.mark.gpu
def test_gpu_soft_selection(gctx, ensemble_iq):
    """Ranges from bit 0, to bit 230400 and across a symbol boundary: selected bits match the reference, every other
    byte keeps its sentinel (-128, a value the quantiser never writes); the correlations cover every symbol."""
    torch, dev = _torch()
    frames, fo = open_loop_frames(ensemble_iq, 8.0)
    idx = [2, 5, 8]
    n = len(idx)
    ranges = [(0, 2048), (5 * 3072 - 160, 320), (40 * 3072 + 16, 3072 * 2), (R.NB_FRAME_BITS - 4096, 4096)]
    keep = np.zeros(R.NB_FRAME_BITS, bool)
    for a, c in ranges:
        keep[a:a + c] = True
    d_iq = torch.from_numpy(np.ascontiguousarray(frames[idx])).to(dev)
    d_fo = torch.from_numpy(np.ascontiguousarray(fo[idx])).to(dev)
    soft = torch.full((n, R.NB_FRAME_BITS), -128, dtype=torch.int8, device=dev)
    cyc = torch.zeros((n, 76), dtype=torch.complex64, device=dev)
    gctx.set_soft_selection(ranges)
    try:
        gctx.ofdm_demod_frames_dev(d_iq.data_ptr(), FRAME, n, d_fo.data_ptr(), soft.data_ptr(), cyc.data_ptr())
        gctx.sync()
    finally:
        gctx.set_soft_selection(None)
    s, cy = soft.cpu().numpy(), cyc.cpu().numpy()
    for k, i in enumerate(idx):
        assert (s[k][~keep] == -128).all(), "bytes outside the selection were written"
        fr = R.Frame(frames[i], fo[i])
        check_cyc(cy[k], fr, "selection")
        filled = np.where(keep, s[k], fr.soft())          # unselected bits replaced by the reference's own
        check_soft(filled, fr, "selection frame %d" % i, 8.0)


# measured on the MI355X with the seeded 8 dB frame below; include/dabgpu.h states it
SCALE_RANGE = (-52, 56)


@pytest.mark.gpu
def test_gpu_power_of_two_scaling_is_bit_identical(gctx, ensemble_iq):
    """x 2^k for k in SCALE_RANGE (unit mean sample power) changes no soft bit: every step is scale-free and exact for a
    power of two until float32 over- or underflows or the quantiser's 1e-30 floor is reached."""
    frames, fo = open_loop_frames(ensemble_iq, 8.0)
    x, f = frames[3], fo[3]
    ks = np.arange(-70, 71)
    batch = np.stack([(x * np.float32(2.0 ** int(k))).astype(np.complex64) for k in ks])
    soft, _, _ = gctx.ofdm_demod_frames(batch, np.full(len(ks), f, np.float32))
    base = soft[ks == 0][0]
    check_soft(base, R.Frame(x, f), "scaling base", 8.0)
    same = np.array([(s == base).all() for s in soft])
    lo = hi = 0
    while lo - 1 >= ks[0] and same[ks == lo - 1][0]:
        lo -= 1
    while hi + 1 <= ks[-1] and same[ks == hi + 1][0]:
        hi += 1
    print("power-of-two scaling: bit-identical for k in [%d, %d]" % (lo, hi))
    assert lo <= SCALE_RANGE[0] and hi >= SCALE_RANGE[1], (lo, hi)



@pytest.mark.gpu
def test_gpu_zero_symbol_erases_its_two_differential_symbols(gctx, ensemble_iq):
    frames, fo = open_loop_frames(ensemble_iq, 20.0)
    x = frames[5].copy()
    l0 = 37
    x[l0 * R.NB_SYM:(l0 + 1) * R.NB_SYM] = 0
    soft, cyc, _ = gctx.ofdm_demod_frames(x[None], fo[5:6], want_cyc=True)
    fr = R.Frame(x, fo[5])
    rows = soft[0].reshape(R.NB_DATA_SYMBOLS, R.NB_SYM_BITS)
    assert not rows[l0 - 1].any() and not rows[l0].any()
    assert fr.erased()[l0 - 1].all() and fr.erased()[l0].all() and not fr.erased()[:l0 - 1].any()
    others = np.r_[0:l0 - 1, l0 + 1:R.NB_DATA_SYMBOLS]
    check_soft(soft[0], fr, "zero symbol %d" % l0, 20.0, rows=others)
    check_soft(soft[0], fr, "zero symbol, all rows")
    assert cyc[0][l0] == 0
    check_cyc(cyc[0], fr, "zero symbol")
