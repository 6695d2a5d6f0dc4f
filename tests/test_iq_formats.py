"""Integer sample formats (dabgpu_set_iq_format): cs16, cs8 and cu8 read by the device-pointer calls and the ring.

The contract is bit-exactness: every output on integer samples equals what the cf32 path produces on a float32 buffer
holding the same values (float(i), float(q); cu8: u - 127.5).  So each GPU test runs the same call sequence on two contexts
-- one fed the integers, one fed their float32 values -- and compares bytes.  The CPU part holds the new front-end
instantiations to the register budget the cf32 ones keep."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

L = 196608                     # samples per transmitted frame
NULL = 2656
SYMS = 76 * 2552               # samples the demodulator reads per frame
FORMATS = ("cs16", "cs8", "cu8")
CSRC = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "csrc")


# ------------------------------------------------------------------------------------------------------------ helpers
def quantise(x, fmt, rms=None):
    """complex64 samples -> (integer samples [..., 2] of format `fmt`, the float32 complex values they stand for)."""
    v = np.stack([x.real, x.imag], axis=-1).astype(np.float64)
    if rms is None:
        rms = {"cs16": 2000.0, "cs8": 25.0, "cu8": 25.0}[fmt]
    v *= rms / max(float(np.sqrt(np.mean(v * v))), 1e-30)
    if fmt == "cs16":
        q = np.clip(np.rint(v), -32768, 32767).astype(np.int16)
        f = q.astype(np.float32)
    elif fmt == "cs8":
        q = np.clip(np.rint(v), -128, 127).astype(np.int8)
        f = q.astype(np.float32)
    else:
        q = np.clip(np.rint(v + 127.5), 0, 255).astype(np.uint8)
        f = q.astype(np.float32) - np.float32(127.5)
    return q, np.ascontiguousarray(f).view(np.complex64)[..., 0]


def fmt_code(fmt):
    import dabgpu
    return {"cs16": dabgpu.IQ_CS16, "cs8": dabgpu.IQ_CS8, "cu8": dabgpu.IQ_CU8}[fmt]


def sample_bytes(fmt):
    return {"cs16": 4, "cs8": 2, "cu8": 2, "cf32": 8}[fmt]


def frames_of(seed, n_frames, snr=15.0, cfo_carriers=0.37, ppm=0.0):
    """n_frames of a cyclic 4-frame multiplex through a channel (CFO, noise, an echo) -> ([n_frames][SYMS] PRS-aligned, ens)."""
    from dabgpu import synth
    e = synth.Ensemble(seed=seed, n_frames=4)
    tx = np.tile(e.iq().ravel(), (n_frames + 3) // 4)[:n_frames * L]
    rng = np.random.default_rng(seed)
    x = synth.channel(tx, snr_db=snr, cfo=cfo_carriers / 2048.0, rng=rng, sco_ppm=ppm, paths=[(0, 1.0), (37, 0.3j)])
    return np.ascontiguousarray(x.reshape(n_frames, L)[:, NULL:NULL + SYMS]), e


def layout(frames, stride):
    """[n][SYMS] -> [n][stride] (zero padding behind every frame)."""
    out = np.zeros((frames.shape[0], stride) + frames.shape[2:], frames.dtype)
    out[:, :SYMS] = frames
    return out


@pytest.fixture(scope="module")
def pair(built):
    """(cf32 context, integer context): the second one's format is set by each test."""
    from conftest import make_ctx
    ref, got = make_ctx(None, 64), make_ctx(None, 64)
    yield ref, got
    got.close()
    ref.close()


def states(torch, ctx, n):
    import dabgpu
    t = dabgpu.device_tensor(torch, ctx.stream_states_ptr, (n * 64,), torch.uint8, torch.device("cuda", 0))
    return t.cpu().numpy().copy()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def selection_ranges():
    """FIC + the 64 kbps sub-channel at CU 0 of every CIF (frame-bit coordinates)."""
    import dabgpu
    sc = dabgpu.subchannel(0, 64, level=3)
    return [(0, 9216)] + [(9216 + c * 55296 + sc.start_address * 64, sc.length * 64) for c in range(4)]


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("odd", [False, True], ids=["even_stride", "odd_stride"])
def test_gpu_streams_closed_loop_bit_exact(pair, fmt, odd):
    """ofdm_demod_streams_dev, 2 streams x 16 frames, three consecutive calls, cyclic-prefix and decision-directed loop, all
    soft bits and then FIC + one sub-channel: soft bits, correlations and stream states equal the cf32 path's after every
    call.  An odd frame_stride puts every other frame at an odd sample (the per-sample loads); the cf32 reference, which
    needs an even stride, holds the same frames at stride + 1."""
    import torch
    import dabgpu
    ref, got = pair
    S, F = 2, 16
    fr = np.concatenate([frames_of(100 + s, F, cfo_carriers=0.2 + 0.3 * s)[0] for s in range(S)])
    q, f = quantise(fr, fmt)
    stride = SYMS + 1000 + (1 if odd else 0)
    d_q, d_f = to_dev(torch, layout(q, stride)), to_dev(torch, layout(f, stride + (stride & 1)))
    got.set_iq_format(fmt_code(fmt))
    try:
        for sel in (None, selection_ranges()):
            for dd in (False, True):
                for c in (ref, got):
                    c.set_soft_selection(sel)
                    c.set_stream_loop(decision_directed=dd)
                    c.streams_reset(S)
                outs = {}
                for name, c, d, st in (("ref", ref, d_f, stride + (stride & 1)), ("got", got, d_q, stride)):
                    soft = torch.full((S * F, dabgpu.NB_FRAME_BITS), 0x5A, dtype=torch.int8, device=d.device)
                    cyc = None if dd else torch.zeros((S * F, 76), dtype=torch.complex64, device=d.device)
                    rec = []
                    for call in range(3):
                        c.ofdm_demod_streams_dev(d.data_ptr(), st, S, F, 0.9, soft.data_ptr(), None if cyc is None else cyc.data_ptr())
                        c.sync()
                        rec.append((soft.cpu().numpy().copy(), None if cyc is None else cyc.cpu().numpy().view(np.uint32).copy(),
                                    states(torch, c, S)))
                    outs[name] = rec
                for call in range(3):
                    (sr, cr, str_), (sg, cg, stg) = outs["ref"][call], outs["got"][call]
                    what = (fmt, odd, sel is not None, dd, call)
                    assert (sr == sg).all(), what
                    assert cr is None or (cr == cg).all(), what
                    assert (str_ == stg).all(), what
                assert (outs["got"][2][0] != 0x5A).any()
    finally:
        for c in (ref, got):
            c.set_soft_selection(None)
            c.set_stream_loop(decision_directed=False)
        got.set_iq_format(dabgpu.IQ_CF32)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_open_loop_frames_bit_exact(pair, fmt):
    """ofdm_demod_frames_dev with per-frame offsets and with freq_offset = NULL (the kernel without the NCO), cyclic-prefix
    correlations on, at an even and an odd frame_stride; ofdm_demod_frames_dd_dev; sync_prs_dev."""
    import torch
    import dabgpu
    ref, got = pair
    n = 6
    fr, _ = frames_of(7, n, cfo_carriers=0.0)
    q, f = quantise(fr, fmt)
    fo = to_dev(torch, np.linspace(-3e-4, 2e-4, n).astype(np.float32))
    got.set_iq_format(fmt_code(fmt))
    try:
        for stride in (SYMS + 64, SYMS + 65):
            d_q, d_f = to_dev(torch, layout(q, stride)), to_dev(torch, layout(f, stride + (stride & 1)))
            res = {}
            for name, c, d, st in (("ref", ref, d_f, stride + (stride & 1)), ("got", got, d_q, stride)):
                r = []
                for p_fo in (fo.data_ptr(), None):
                    soft = torch.zeros((n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=d.device)
                    cyc = torch.zeros((n, 76), dtype=torch.complex64, device=d.device)
                    c.ofdm_demod_frames_dev(d.data_ptr(), st, n, p_fo, soft.data_ptr(), cyc.data_ptr())
                    dd4 = torch.zeros((n, 76), dtype=torch.complex64, device=d.device)
                    soft2 = torch.zeros_like(soft)
                    c.ofdm_demod_frames_dd_dev(d.data_ptr(), st, n, p_fo, soft2.data_ptr(), dd4.data_ptr())
                    sync = torch.zeros((n, 4), dtype=torch.int32, device=d.device)
                    c.sync_prs_dev(d.data_ptr(), st, n, p_fo, 8 if p_fo is None else 0, sync.data_ptr())
                    c.sync()
                    r += [soft.cpu().numpy(), cyc.cpu().numpy().view(np.uint32), soft2.cpu().numpy(), dd4.cpu().numpy().view(np.uint32),
                          sync.cpu().numpy()]
                res[name] = r
            for k, (a, b) in enumerate(zip(res["ref"], res["got"])):
                assert (a == b).all(), (fmt, stride, k)
            assert res["got"][0].any() and res["got"][2].any()
    finally:
        got.set_iq_format(dabgpu.IQ_CF32)


def capture(seed, n_frames, ppm, cfo_carriers, snr, cut):
    """a stream of n_frames through a channel with a sample-clock offset, cut `cut` samples into frame 0 -> (iq, ensemble)"""
    from dabgpu import synth
    e = synth.Ensemble(seed=seed, n_frames=4)
    tx = np.tile(e.iq().ravel(), (n_frames + 3) // 4)[:n_frames * L]
    x = synth.channel(tx, snr_db=snr, cfo=cfo_carriers / 2048.0, rng=np.random.default_rng(seed), sco_ppm=ppm)
    return x[cut:], e


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_acquire_and_track_bit_exact(pair, fmt):
    """Unaligned captures at +-100 ppm (odd cuts: frames at odd samples): acquire_dev -> ofdm_demod_acquired_dev ->
    track_start_dev -> two ofdm_demod_tracked_dev calls, then the same from fresh states with cfg.auto_acquire.  Frame
    records, counts, soft bits, correlations and states equal the cf32 path's."""
    import torch
    import dabgpu
    ref, got = pair
    specs = [(100.0, 1.7, 16.0, 41001), (-100.0, -2.3, 14.0, 77777)]
    caps = [capture(60 + i, 10, *sp)[0] for i, sp in enumerate(specs)]
    n_total = min(c.size for c in caps)
    x = np.stack([c[:n_total] for c in caps])
    q, f = quantise(x, fmt)
    S, MF, n_cap, adv = 2, 4, 3 * L + 8192, 2 * L
    d_q, d_f = to_dev(torch, q), to_dev(torch, f)
    got.set_iq_format(fmt_code(fmt))
    try:
        for auto in (False, True):
            res = {}
            for name, c, d, sb in (("ref", ref, d_f, 8), ("got", got, d_q, sample_bytes(fmt))):
                dev = d.device
                c.streams_reset(S)
                frames = torch.zeros((S, MF, 32), dtype=torch.uint8, device=dev)
                counts = torch.zeros(S, dtype=torch.int32, device=dev)
                soft = torch.zeros((S * MF, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
                cyc = torch.zeros((S * MF, 76), dtype=torch.complex64, device=dev)
                r = []
                if not auto:
                    c.acquire_dev(d.data_ptr(), n_total, S, n_cap, MF, frames.data_ptr(), counts.data_ptr())
                    c.ofdm_demod_acquired_dev(d.data_ptr(), n_total, S, MF, frames.data_ptr(), soft.data_ptr(), d_cyc=cyc.data_ptr())
                    c.track_start_dev(frames.data_ptr(), counts.data_ptr(), S, MF, adv)
                    calls = [adv, 2 * adv]
                else:
                    calls = [0, adv, 2 * adv]
                c.sync()
                r += [frames.cpu().numpy().copy(), counts.cpu().numpy().copy(), soft.cpu().numpy().copy(), states(torch, c, S)]
                cfg = dabgpu.track_cfg(auto_acquire=1) if auto else None
                for base in calls:
                    c.ofdm_demod_tracked_dev(d.data_ptr() + base * sb, n_total, S, n_cap, MF, adv, soft.data_ptr(), frames.data_ptr(),
                                             counts.data_ptr(), cfg=cfg, d_cyc=cyc.data_ptr())
                    c.sync()
                    r += [frames.cpu().numpy().copy(), counts.cpu().numpy().copy(), soft.cpu().numpy().copy(),
                          cyc.cpu().numpy().view(np.uint32).copy(), states(torch, c, S)]
                res[name] = r
            for k, (a, b) in enumerate(zip(res["ref"], res["got"])):
                assert (a == b).all(), (fmt, auto, k)
            cnt = res["got"][-4]
            assert (cnt >= 2).all(), cnt
            fr = res["got"][-5].view(dabgpu.ACQUIRED_FRAME_DTYPE).reshape(S, MF)
            assert (fr[:, :2]["flags"] == 3).all()
        # sync_prs_dev on the last call's two frames where they lie (any sample offset, any stride); the cf32 reference,
        # which needs 16-byte alignment and an even stride, gets the same samples copied into rows of 2552
        starts = fr[0, :2]["start"].astype(np.int64) + 2 * adv
        rows = np.stack([f[0, s0:s0 + 2552] for s0 in starts])
        d_rows = to_dev(torch, rows)
        res = {}
        for name, c, p, st in (("ref", ref, d_rows.data_ptr(), 2552),
                               ("got", got, d_q.data_ptr() + int(starts[0]) * sample_bytes(fmt), int(starts[1] - starts[0]))):
            out = torch.zeros((2, 4), dtype=torch.int32, device=d_q.device)
            c.sync_prs_dev(p, st, 2, None, 16, out.data_ptr())
            c.sync()
            res[name] = out.cpu().numpy()
        assert (res["ref"] == res["got"]).all()
    finally:
        got.set_iq_format(dabgpu.IQ_CF32)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_ring_bit_exact(pair, fmt):
    """The host-fed ring on integer samples: open-loop and closed-loop submits over three batches; FIBs, CRC flags,
    sub-channel bytes and soft bits equal a cf32 ring's on the same values."""
    import dabgpu
    ref, got = pair
    n, batch = 12, 4
    fr, _ = frames_of(21, n)
    q, f = quantise(fr, fmt)
    sc = dabgpu.subchannel(0, 64, level=3)
    got.set_iq_format(fmt_code(fmt))
    try:
        for closed in (False, True):
            res = {}
            for name, c, iq in (("ref", ref, f), ("got", got, q)):
                c.streams_reset(1)
                c.pipe_open(3, batch, SYMS)
                fo = np.full(n, -0.37 / 2048, np.float32)
                soft = np.zeros((n, dabgpu.NB_FRAME_BITS), np.int8)
                fib = np.zeros((n, 12, 32), np.uint8)
                ok = np.zeros((n, 12), np.uint8)
                out = np.zeros((n * 4, 192), np.uint8)
                ts = []
                for lo in range(0, n, batch):
                    ts.append(c.pipe_submit(iq[lo:lo + batch], 1, batch, None if closed else fo[lo:lo + batch], [sc], soft[lo:lo + batch],
                                            fib[lo:lo + batch], ok[lo:lo + batch], [out[4 * lo:4 * lo + 4 * batch]]))
                for t in ts:
                    c.pipe_wait(t)
                c.pipe_close()
                res[name] = (soft, fib, ok, out)
            for k, (a, b) in enumerate(zip(res["ref"], res["got"])):
                assert (a == b).all(), (fmt, closed, k)
            assert res["got"][2][batch if closed else 0:].all()         # (the closed loop pulls in over its first batch)
    finally:
        got.set_iq_format(dabgpu.IQ_CF32)


@pytest.mark.gpu
def test_gpu_cu8_capture_decodes(pair):
    """A 20 dB capture quantised to cu8 at ~25 counts RMS (an rtl_sdr's view of it), acquired, demodulated, tracked and
    decoded: every FIB's CRC passes, the FIBs and the 64 kbps sub-channel's logical frames are the transmitted ones."""
    import torch
    import dabgpu
    _, got = pair
    x, e = capture(5, 10, 0.0, 0.8, 20.0, 50001)
    q, _ = quantise(x, "cu8", rms=25.0)
    d_q = to_dev(torch, q)
    n_cap, MF = 6 * L, 8
    sc = dabgpu.subchannel(0, 64, level=3)
    got.set_iq_format(dabgpu.IQ_CU8)
    try:
        got.streams_reset(1)
        dev = d_q.device
        frames = torch.zeros((1, MF, 32), dtype=torch.uint8, device=dev)
        counts = torch.zeros(1, dtype=torch.int32, device=dev)
        soft = torch.zeros((MF, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
        got.acquire_dev(d_q.data_ptr(), q.shape[0], 1, n_cap, MF, frames.data_ptr(), counts.data_ptr())
        got.ofdm_demod_acquired_dev(d_q.data_ptr(), q.shape[0], 1, MF, frames.data_ptr(), soft.data_ptr())
        got.track_start_dev(frames.data_ptr(), counts.data_ptr(), 1, MF, 2 * L)
        got.sync()
        cnt = int(counts.cpu().numpy()[0])
        assert cnt >= 5, cnt
        fr = frames.cpu().numpy().view(dabgpu.ACQUIRED_FRAME_DTYPE).reshape(MF)
        assert (fr[:cnt]["flags"] == 3).all()
        s = soft.cpu().numpy()[:cnt]
        fib, ok, (msc,), _ = got.decode_frames(s, 1, [sc])
        assert ok.all()
        k0 = [k for k in range(4) if (fib[0] == e.fibs[k]).all()]
        assert len(k0) == 1, "first acquired frame is no transmitted frame"
        k0 = k0[0]
        for j in range(cnt):
            assert (fib[j] == e.fibs[(k0 + j) % 4]).all(), j
        checked = 0
        for cif in range(15, 4 * cnt):
            assert (msc[0, cif] == e.msc_bytes[(4 * k0 + cif - 15) % 16]).all(), cif
            checked += 1
        assert checked >= 5
        # ... and one tracked call on the capture that begins two frames on: the frames behind the acquired ones decode as well
        soft.zero_()
        got.ofdm_demod_tracked_dev(d_q.data_ptr() + 2 * L * 2, q.shape[0], 1, q.shape[0] - 2 * L, MF, 2 * L, soft.data_ptr(),
                                   frames.data_ptr(), counts.data_ptr())
        got.sync()
        cnt = int(counts.cpu().numpy()[0])
        assert cnt >= 2, cnt
        fib, ok, _, _ = got.decode_frames(soft.cpu().numpy()[:cnt], 1, [])
        assert ok.all()
    finally:
        got.set_iq_format(dabgpu.IQ_CF32)


@pytest.mark.gpu
def test_gpu_defaults_and_refusals(pair):
    """A fresh context reads cf32 (the same bytes before and after set_iq_format(IQ_CF32)); an unknown format, a format
    change under an open ring, and every cf32-only entry point on an integer context are refused with ERR_ARG and leave a
    sentinel-filled output untouched."""
    import ctypes as C
    import torch
    import dabgpu
    ref, got = pair
    ERR_ARG = -1
    fr, _ = frames_of(3, 2)
    d_f = to_dev(torch, fr)
    dev = d_f.device
    assert got.iq_format == dabgpu.IQ_CF32
    outs = []
    for k in range(2):
        soft = torch.zeros((2, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
        got.ofdm_demod_frames_dev(d_f.data_ptr(), SYMS, 2, None, soft.data_ptr())
        got.sync()
        outs.append(soft.cpu().numpy())
        got.set_iq_format(dabgpu.IQ_CF32)
    assert (outs[0] == outs[1]).all() and outs[0].any()
    lib, h = got._lib, got._h
    for bad in (-1, 4, 99):
        assert lib.dabgpu_set_iq_format(h, bad) == ERR_ARG
    assert got.iq_format == dabgpu.IQ_CF32
    # an open ring keeps its format
    got.pipe_open(2, 1, SYMS)
    try:
        assert lib.dabgpu_set_iq_format(h, dabgpu.IQ_CU8) == ERR_ARG
        assert got.iq_format == dabgpu.IQ_CF32
    finally:
        got.pipe_close()
    q, _ = quantise(fr, "cs16")
    d_q = to_dev(torch, q)
    got.set_iq_format(dabgpu.IQ_CS16)
    try:
        got.streams_reset(1)
        S8 = 0x5A
        host_iq = np.ascontiguousarray(fr)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        soft_h = np.full((2, dabgpu.NB_FRAME_BITS), S8, np.int8)
        spec_h = np.full((2, 76, 2048), 7, np.complex64)
        sync_h = np.full((2, 4), S8, np.int32)
        acq_h = np.full((1, 4, 32), S8, np.uint8)
        cnt_h = np.full(1, S8, np.int32)
        soft_d = torch.full((2, dabgpu.NB_FRAME_BITS), S8, dtype=torch.int8, device=dev)
        dq_d = torch.full((2, 75, 1536), 7, dtype=torch.complex64, device=dev)
        spec_d = torch.full((2, 76, 2048), 7, dtype=torch.complex64, device=dev)
        acq_d = torch.full((1, 4, 32), S8, dtype=torch.uint8, device=dev)
        cnt_d = torch.full((1,), S8, dtype=torch.int32, device=dev)
        res = dabgpu.FrameResult()
        rcs = {
            "ofdm_demod_frames": lib.dabgpu_ofdm_demod_frames(h, p(host_iq), SYMS, 2, None, p(soft_h), None, None),
            "ofdm_demod_streams": lib.dabgpu_ofdm_demod_streams(h, p(host_iq), SYMS, 1, 2, 0.9, p(soft_h), None, None),
            "fft_symbols": lib.dabgpu_fft_symbols(h, p(host_iq), SYMS, 2, None, p(spec_h)),
            "sync_prs": lib.dabgpu_sync_prs(h, p(host_iq), SYMS, 2, None, 8, p(sync_h)),
            "acquire": lib.dabgpu_acquire(h, p(host_iq), 2 * SYMS, 1, 2 * SYMS, None, 4, p(acq_h), p(cnt_h)),
            "ofdm_demod_stream_frame": lib.dabgpu_ofdm_demod_stream_frame(h, 0, p(host_iq), 1, None, p(soft_h), None, C.byref(res)),
            "fft_symbols_dev": lib.dabgpu_fft_symbols_dev(h, d_q.data_ptr(), SYMS, 2, None, spec_d.data_ptr(), None),
            "mover_frames_dev": lib.dabgpu_mover_frames_dev(h, d_q.data_ptr(), SYMS, 2, soft_d.data_ptr(), 0, None),
            "frames_dev+dqpsk": lib.dabgpu_ofdm_demod_frames_dev(h, d_q.data_ptr(), SYMS, 2, None, soft_d.data_ptr(), None,
                                                                 dq_d.data_ptr(), None),
            "streams_dev+dqpsk": lib.dabgpu_ofdm_demod_streams_dev(h, d_q.data_ptr(), SYMS, 1, 2, 0.9, soft_d.data_ptr(), None,
                                                                   dq_d.data_ptr(), None),
            "acquired_dev+dqpsk": lib.dabgpu_ofdm_demod_acquired_dev(h, d_q.data_ptr(), 2 * SYMS, 1, 4, acq_d.data_ptr(),
                                                                     soft_d.data_ptr(), None, dq_d.data_ptr(), None),
            "tracked_dev+dqpsk": lib.dabgpu_ofdm_demod_tracked_dev(h, d_q.data_ptr(), 2 * SYMS, 1, 2 * SYMS, 4, L, None,
                                                                   soft_d.data_ptr(), None, dq_d.data_ptr(), acq_d.data_ptr(),
                                                                   cnt_d.data_ptr(), None),
        }
        got.sync()
        for k, rc in rcs.items():
            assert rc == ERR_ARG, (k, rc)
        assert (soft_h == S8).all() and (spec_h == 7).all() and (sync_h == S8).all() and (acq_h == S8).all() and (cnt_h == S8).all()
        assert (soft_d.cpu().numpy() == S8).all() and (dq_d.cpu().numpy() == 7).all() and (spec_d.cpu().numpy() == 7).all()
        assert (acq_d.cpu().numpy() == S8).all() and (cnt_d.cpu().numpy() == S8).all()
        # a cs16 pointer must hold one sample of alignment
        assert lib.dabgpu_ofdm_demod_frames_dev(h, d_q.data_ptr() + 2, SYMS, 2, None, soft_d.data_ptr(), None, None, None) == ERR_ARG
        # the ring checks the dtype of what it is given
        got.pipe_open(2, 1, SYMS)
        try:
            fib = np.zeros((1, 12, 32), np.uint8)
            ok = np.zeros((1, 12), np.uint8)
            with pytest.raises(ValueError):
                got.pipe_submit(host_iq[:1], 1, 1, np.zeros(1, np.float32), [], None, fib, ok, [])
        finally:
            got.pipe_close()
    finally:
        got.set_iq_format(dabgpu.IQ_CF32)


# ------------------------------------------------------------------------------------------------------------ CPU
def device_asm(tmp_path_factory, src):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the device assembly cannot be checked")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    out = tmp_path_factory.mktemp("iq_asm") / (src + ".s")
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, src + ".hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def test_integer_front_end_instantiations_keep_the_register_budget(tmp_path_factory):
    """Every integer-format instantiation of ofdm_wave_kernel -- fused, {plain, selection} x {NCO, none} x {cs16, cs8, cu8} --
    exists with 0 spills, no scratch, <= 168 VGPRs and <= 160 KB / 3 of LDS (three 4-wave workgroups per CU, as cf32)."""
    from test_device_asm import kernel_metadata
    md = kernel_metadata(device_asm(tmp_path_factory, "ofdm_kernels"))
    want = {"ILb0ELb0ELb%dELb%dELi%dEE" % (sel, nco, f) for sel in (0, 1) for nco in (0, 1) for f in (1, 2, 3)}
    got = {}
    for k, v in md.items():
        m = re.search(r"ofdm_wave_kernel(ILb\dELb\dELb\dELb\dELi\dEE)", k)
        if m and not m.group(1).endswith("Li0EE"):
            got[m.group(1)] = v
    assert set(got) == want, set(got) ^ want
    for k, v in got.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_count"] <= 168 and v.get("agpr_count", 0) == 0, (k, v)
        assert v["group_segment_fixed_size"] <= 160 * 1024 // 3, (k, v)
    su = [v for k, v in md.items() if re.search(r"stream_update_kernelILi[123]E", k)]
    assert len(su) == 3 and all(v["private_segment_fixed_size"] == 0 for v in su)


def test_integer_sync_kernels_gain_no_scratch(tmp_path_factory):
    """The sample-reading sync kernels on integer formats use no more scratch than their cf32 twins (prs_sync_kernel in
    tracking mode already has 144 B) and spill no more registers."""
    from test_device_asm import kernel_metadata
    md = kernel_metadata(device_asm(tmp_path_factory, "sync_kernels"))
    checked = 0
    for k, v in md.items():
        m = re.search(r"(prs_sync_kernelILi\dELb\d|null_l1_kernel|track_update_kernel)(E?)ILi([123])E|"
                      r"(prs_sync_kernelILi\dELb\d)ELi([123])E", k)
        if not m:
            continue
        if m.group(4):
            twin = [w for kk, w in md.items() if m.group(4) + "ELi0E" in kk]
        else:
            twin = [w for kk, w in md.items() if m.group(1) + "ILi0E" in kk]
        assert len(twin) == 1, k
        assert v["private_segment_fixed_size"] <= twin[0]["private_segment_fixed_size"], (k, v, twin[0])
        assert v["vgpr_spill_count"] <= twin[0]["vgpr_spill_count"] and v["sgpr_spill_count"] <= twin[0]["sgpr_spill_count"], (k, v)
        checked += 1
    assert checked == 3 * 3 + 3 + 3, checked                   # prs_sync (plain, acquire, lite tracking), null_l1, track_update
