"""Channel impulse response from the phase reference symbol (include/dabgpu.h, "Channel impulse response").  The CPU tests
check the binding's layouts, the host analysis rule and the float64 reference itself; the GPU tests hold the kernel's
per-frame records and sums to tests/cir_reference.py and recover known channels from them."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth
from conftest import ROOT, make_ctx
import cir_reference as R

CSRC = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "csrc")
SYM = synth.NB_SYM
NULL = synth.NB_NULL
REC = dabgpu.CIR_ACC_DTYPE.itemsize


def acc_of(tap, frames=1):
    a = np.zeros((), dabgpu.CIR_ACC_DTYPE)
    a["tap"] = tap
    a["frames"] = frames
    return a


def paths_of(out):
    return [(float(p["delay"]), float(p["level_db"]), float(p["snr_db"]), bool(p["flags"] & dabgpu.CIR_BEYOND_GUARD)) for p in out]


def agree(acc, frames, min_snr_db=10.0, range_db=25.0):
    """the library's analysis equals the reference's (float32 outputs of float64 arithmetic)"""
    rep, out = dabgpu.cir_analyse(acc, min_snr_db=min_snr_db, range_db=range_db, max_out=2048)
    wrep, wpaths = R.analyse(acc["tap"], frames, min_snr_db, range_db)
    got = paths_of(out)
    assert int(rep["n_paths"]) == wrep["n_paths"] == len(got) == len(wpaths)
    assert int(rep["frames"]) == frames
    for f in ("floor", "peak", "first_delay", "strongest_delay", "rms_delay_spread", "guard_ratio_db"):
        w = wrep[f]
        if math.isinf(w):
            assert float(rep[f]) == w, f
        else:
            assert abs(float(rep[f]) - w) <= 1e-6 * max(1.0, abs(w)), (f, float(rep[f]), w)
    for g, w in zip(got, wpaths):
        assert g[3] == w[3]
        for a, b in zip(g[:3], w[:3]):
            assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (g, w)
    return rep, got


# ------------------------------------------------------------------ layouts
def test_cir_structures_match_the_header(tmp_path, built):
    pairs = [("dabgpu_cir_acc", dabgpu.CIR_ACC_DTYPE), ("dabgpu_cir_report", dabgpu.CIR_REPORT_DTYPE),
             ("dabgpu_cir_path", dabgpu.CIR_PATH_DTYPE)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dabgpu.h"', 'int main(void) {']
    for cname, dt in pairs:
        lines.append('  printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for f in dt.names:
            lines.append('  printf(" %%zu", offsetof(%s, %s));' % (cname, f))
        lines.append('  printf("\\n");')
    lines.append('  printf("cfg %zu %zu %zu %d\\n", sizeof(dabgpu_cir_cfg), offsetof(dabgpu_cir_cfg, min_snr_db), '
                 'offsetof(dabgpu_cir_cfg, range_db), DABGPU_CIR_BEYOND_GUARD);')
    lines.append('  return 0; }')
    src = tmp_path / "cir_layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "cir_layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    for (cname, dt), line in zip(pairs, out):
        got = line.split()
        assert got[0] == cname
        assert [int(x) for x in got[1:]] == [dt.itemsize] + [dt.fields[f][1] for f in dt.names], (cname, got)
    assert out[3].split() == ["cfg", str(dabgpu.C.sizeof(dabgpu.CirCfg)), str(dabgpu.CirCfg.min_snr_db.offset),
                              str(dabgpu.CirCfg.range_db.offset), str(dabgpu.CIR_BEYOND_GUARD)]
    assert REC == 14352
    cfg = dabgpu.CirCfg()
    dabgpu.lib().dabgpu_cir_default_cfg(dabgpu.C.byref(cfg))
    assert cfg.min_snr_db == 10.0 and cfg.range_db == 25.0


def test_unit_helpers():
    assert dabgpu.samples_to_us(2048) == 1000.0
    assert abs(dabgpu.samples_to_us(504) - 246.09375) < 1e-12
    assert abs(dabgpu.samples_to_km(2.048) - 0.299792458) < 1e-12
    assert np.allclose(dabgpu.samples_to_km(np.array([0.0, 504.0])), [0.0, 504 / 2.048 * 0.299792458])


# ------------------------------------------------------------------ the reference itself
def prs_symbol():
    """the 2552 samples of the PRS (prefix + useful part), unit mean power, float64 from synth.prs_carriers()"""
    Z = np.zeros(2048, np.complex128)
    Z[R.BINS] = R.prs() * (2048 / np.sqrt(1536))
    u = np.fft.ifft(Z)
    return np.concatenate([u[-504:], u])


def test_reference_unit_path_and_flat_channel():
    """Noise-free, float64: a unit path at integer delay d gives tap[d] = 1; a flat channel gives carrier = 1."""
    prs = prs_symbol()
    assert abs(np.mean(np.abs(prs[504:]) ** 2) - 1.0) < 1e-9
    assert abs(R.S - 768.0) < 1e-9
    tap, car = R.record(prs[504:2552])
    assert abs(tap[0] - 1.0) < 1e-9 and np.all(np.abs(car - 1.0) < 1e-9)
    for d, g in ((7, 1.0), (213, 1j), (504, -1.0)):
        y = np.zeros(2 * SYM, np.complex128)
        y[d:d + SYM] = g * prs                           # delayed: the window starts d samples into the prefix
        tap, car = R.record(y[504:2552])
        assert abs(tap[d] - 1.0) < 1e-9 and tap.argmax() == d, d
        assert np.all(np.abs(car - 1.0) < 1e-9)
        # far from the path every tap is the DC hole's -57.7 dB or less
        far = np.abs(((np.arange(2048) - d + 1024) % 2048) - 1024) > 4
        assert tap[far].max() < 10 ** -4.5
    # an early arrival reads as a negative delay (tap 2048 - 5): the useful part seen 5 samples late, cyclically
    tap, _ = R.record(np.roll(prs[504:], -5))
    assert tap.argmax() == 2043 and abs(tap[2043] - 1.0) < 1e-9
    # the frequency correction: an offset undone by its negative gives the clean record back
    n = np.arange(2552)
    y = prs * np.exp(2j * np.pi * 3.3 / 2048 * n)
    tap, car = R.record(y[504:2552], -3.3 / 2048)
    assert abs(tap[0] - 1.0) < 1e-5 and np.all(np.abs(car - 1.0) < 1e-5)      # (f is rounded to float32 and 2^-32)


def test_reference_noise_tap_power():
    """The analytic noise tap power against a Monte-Carlo estimate (white noise only)."""
    rng = np.random.default_rng(4)
    sigma2 = 0.3
    taps = []
    for _ in range(64):
        x = np.sqrt(sigma2 / 2) * (rng.standard_normal(2048) + 1j * rng.standard_normal(2048))
        taps.append(R.record(x)[0])
    assert abs(np.mean(taps) / R.noise_tap_power(sigma2) - 1.0) < 0.02


# ------------------------------------------------------------------ host analysis
def shape_path(tap, d, g2):
    """add a path of power g2 at integer tap d with the Hann main lobe's neighbours"""
    side = 10 ** (-3.2881623710731627 / 10)
    for m, v in ((-1, side), (0, 1.0), (1, side)):
        tap[(d + m) % 2048] += g2 * v


def test_analyse_hand_built(built):
    base = np.full(2048, 1e-5)
    # one path
    t = base.copy()
    shape_path(t, 40, 1.0)
    rep, got = agree(acc_of(t.astype(np.float32)), 1)
    assert len(got) == 1 and abs(got[0][0] - 40) < 1e-6 and abs(got[0][1]) < 1e-6 and not got[0][3]
    assert rep["rms_delay_spread"] == 0.0 and math.isinf(rep["guard_ratio_db"]) and rep["guard_ratio_db"] > 0
    assert abs(rep["floor"] - 1e-5 / R.median_of_mean_exponentials(1)) < 1e-10
    # two paths, summed over 8 frames
    t = base.copy()
    shape_path(t, 40, 1.0)
    shape_path(t, 140, 0.25)
    rep, got = agree(acc_of((8 * t).astype(np.float32), 8), 8)
    assert [round(d) for d, *_ in got] == [40, 140] and abs(got[1][1] + 6.0206) < 1e-3
    assert abs(rep["rms_delay_spread"] - 100 * math.sqrt(0.25) / 1.25) < 1e-3
    # a path at a negative delay comes first
    t = base.copy()
    shape_path(t, 0, 1.0)
    shape_path(t, 2048 - 30, 0.5)
    rep, got = agree(acc_of(t.astype(np.float32)), 1)
    assert [round(d) for d, *_ in got] == [-30, 0] and rep["first_delay"] == -30.0 and rep["strongest_delay"] == 0.0
    # a path beyond the guard
    t = base.copy()
    shape_path(t, 10, 1.0)
    shape_path(t, 600, 0.1)
    rep, got = agree(acc_of(t.astype(np.float32)), 1)
    assert [g[3] for g in got] == [False, True] and abs(rep["guard_ratio_db"] - 10.0) < 1e-3
    # exactly 504 after the first is inside
    t = base.copy()
    shape_path(t, 10, 1.0)
    shape_path(t, 514, 0.1)
    rep, got = agree(acc_of(t.astype(np.float32)), 1)
    assert [g[3] for g in got] == [False, False] and math.isinf(rep["guard_ratio_db"])
    # ties between neighbours: the left one of an equal pair is the path, half a sample to the right
    t = base.copy()
    t[99], t[100], t[101], t[102] = 0.1, 1.0, 1.0, 0.1
    rep, got = agree(acc_of(t.astype(np.float32)), 1)
    assert len(got) == 1 and abs(got[0][0] - 100.5) < 1e-6
    # a flat top of three: no tap is strictly above its left neighbour and at least its right -> the first of the run
    t = base.copy()
    t[200:203] = 1.0
    rep, got = agree(acc_of(t.astype(np.float32)), 1)
    assert [round(g[0], 3) for g in got] == [200.5]
    # the thresholds: range_db and min_snr_db
    t = base.copy()
    shape_path(t, 50, 1.0)
    shape_path(t, 300, 10 ** -3)                         # -30 dB: below the 25 dB range
    assert len(agree(acc_of(t.astype(np.float32)), 1)[1]) == 1
    assert len(agree(acc_of(t.astype(np.float32)), 1, range_db=35.0)[1]) == 2
    assert len(agree(acc_of(t.astype(np.float32)), 1, min_snr_db=60.0)[1]) == 0


def test_analyse_matches_reference_on_random_accumulators(built):
    rng = np.random.default_rng(0xC1C)
    for trial in range(200):
        frames = int(rng.integers(1, 300))
        noise = rng.gamma(frames, 1.0, size=2048) * rng.uniform(1e-6, 1e-2)
        t = noise.copy()
        for _ in range(int(rng.integers(0, 6))):
            d = int(rng.integers(2048))
            frac = rng.uniform(-0.5, 0.5)
            g2 = frames * 10 ** rng.uniform(-4, 0)
            for m in range(-3, 4):
                t[(d + m) % 2048] += g2 * np.sinc((m - frac) * 0.75) ** 2
        min_snr = float(rng.choice([10.0, 3.0, 0.0, 20.0]))
        rng_db = float(rng.choice([25.0, 40.0, 10.0]))
        agree(acc_of(t.astype(np.float32), frames), frames, min_snr, rng_db)


def test_analyse_refusals_and_empty(built):
    L = dabgpu.lib()
    t = np.full(2048, 1e-4, np.float32)
    t[100], t[300] = 1.0, 0.5
    a = acc_of(t)
    out = np.zeros(4, dabgpu.CIR_PATH_DTYPE)
    out.view(np.int32)[:] = -7
    rep = np.zeros((), dabgpu.CIR_REPORT_DTYPE)
    rep_bytes = rep.tobytes()
    p = dabgpu._p
    for bad in (dabgpu.CirCfg(float("nan"), 25.0), dabgpu.CirCfg(10.0, float("inf"))):
        assert L.dabgpu_cir_analyse(p(a), dabgpu.C.byref(bad), p(rep), p(out), 4) == -1
    assert L.dabgpu_cir_analyse(None, None, p(rep), p(out), 4) == -1
    assert L.dabgpu_cir_analyse(p(a), None, p(rep), None, 4) == -1
    assert L.dabgpu_cir_analyse(p(a), None, p(rep), p(out), -1) == -1
    assert (out.view(np.int32) == -7).all() and rep.tobytes() == rep_bytes
    # counted, but only max_out written; the report may be NULL; cfg NULL = the defaults
    assert L.dabgpu_cir_analyse(p(a), None, None, p(out), 1) == 2
    assert abs(out[0]["delay"] - 100.0) < 1e-6 and (out[1:].view(np.int32) == -7).all()
    assert L.dabgpu_cir_analyse(p(a), None, p(rep), None, 0) == 2 and rep["n_paths"] == 2
    # frames == 0 and floor <= 0: no paths, every field after peak is 0
    for acc in (acc_of(t, frames=0), acc_of(np.where(np.arange(2048) == 5, 1.0, 0.0).astype(np.float32))):
        r, got = dabgpu.cir_analyse(acc)
        assert len(got) == 0 and r["n_paths"] == 0
        assert r["first_delay"] == r["strongest_delay"] == r["rms_delay_spread"] == r["guard_ratio_db"] == 0.0
    r, _ = dabgpu.cir_analyse(acc_of(t, frames=0))
    assert r["frames"] == 0 and r["floor"] == 0.0 and r["peak"] == 0.0


# ------------------------------------------------------------------ device code
def test_cir_kernels_spill_nothing():
    from test_device_asm import kernel_metadata
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "cir_kernels.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    asm = subprocess.check_output([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "cir_kernels.hip"), "-o", "-"],
                                  stderr=subprocess.DEVNULL, text=True)
    md = {k: v for k, v in kernel_metadata(asm).items() if "cir_" in k}
    assert len(md) == 5, sorted(md)                       # four sample formats + the accumulation
    for k, v in md.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["group_segment_fixed_size"] <= 32 * 1024 + 64, (k, v)     # five workgroups per CU


# ------------------------------------------------------------------ GPU
def packed_prs(rng, chans, frames, stride, snr_db=None, cfo=None):
    """PRS symbols only, one per frame, the first at 0 and then every `stride` samples (zeros between): one stream per entry
    of chans (synth.channel paths, or None), back to back, [len(chans) * frames * stride] complex64; frame (s, f)'s PRS
    prefix is at (s*frames + f) * stride.  cfo: per stream, cycles/sample."""
    prs = prs_symbol()
    out = []
    for s, paths in enumerate(chans):
        x = np.zeros(frames * stride, np.complex128)
        for f in range(frames):
            x[f * stride:f * stride + SYM] = prs
        x = synth.channel(x, snr_db=snr_db, rng=rng, paths=paths, cfo=0.0 if cfo is None else cfo[s])
        out.append(x)
    return np.concatenate(out).astype(np.complex64)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def cir_acc(torch, n, fill=0):
    t = torch.zeros((n, REC), dtype=torch.uint8, device="cuda:0")
    if fill:
        t.fill_(fill)
    return t


def host(t):
    return t.cpu().numpy().view(dabgpu.CIR_ACC_DTYPE).reshape(-1)


def close(rec, taps, cars, tap_budgets, car_budgets):
    """every tap and every carrier within the budget cir_reference.py derives for it (each at most 1e-4 of the record's
    largest tap, carrier)"""
    for r, t, c, tb, cb in zip(np.atleast_1d(rec), np.atleast_2d(taps), np.atleast_2d(cars), np.atleast_2d(tap_budgets),
                               np.atleast_2d(car_budgets)):
        assert np.all(tb <= 1e-4 * t.max()) and np.all(cb <= 1e-4 * c.max())
        assert np.all(np.abs(r["tap"] - t) <= tb)
        assert np.all(np.abs(r["carrier"] - c) <= cb)


def frame_order_sum(records, S, F, calls=1):
    want = np.zeros(S, dabgpu.CIR_ACC_DTYPE)
    for _ in range(calls):
        for s in range(S):
            for f in range(F):
                want[s]["tap"] += records[s * F + f]["tap"]
                want[s]["carrier"] += records[s * F + f]["carrier"]
    return want


@pytest.fixture(scope="module")
def cctx(built):
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.gpu
def test_gpu_records_match_reference_and_sums_repeat(cctx):
    """Per-frame records against the float64 reference at two strides, several streams and offsets of +-3.3 carriers; the
    sums over two calls are the float32 frame-order sums of the records, repeat bit for bit, and are the same without
    d_frame."""
    import torch
    rng = np.random.default_rng(12)
    S, F = 3, 5
    chans = [[(0, 1.0), (23, 0.5)], [(0, 0.7), (5, -0.3j), (310, 0.2)], None]
    cfo = np.array([3.3, -3.3, 0.8]) / 2048
    for stride in (SYM, SYM + 38):
        y = packed_prs(rng, chans, F, stride, snr_db=15.0, cfo=cfo)
        y = np.concatenate([y, np.zeros(SYM, np.complex64)])
        fo = np.repeat(-cfo, F) + rng.uniform(-0.01, 0.01, S * F) / 2048
        starts = [i * stride for i in range(S * F)]
        ref = R.records(y.astype(np.complex128), starts, fo, budgets=True)
        d = dev(torch, y)
        d_fo = dev(torch, fo.astype(np.float32))
        runs = []
        for with_frame in (True, True, False):
            acc = cir_acc(torch, S)
            frame = cir_acc(torch, S * F, fill=0xA5)
            for _ in range(2):
                cctx.cir_frames_dev(d.data_ptr(), stride, S, F, acc.data_ptr(), d_freq_offset=d_fo.data_ptr(),
                                    d_frame=frame.data_ptr() if with_frame else None)
            cctx.sync()
            runs.append((acc.cpu().numpy().copy(), host(frame).copy()))
        fr = runs[0][1]
        close(fr, *ref)
        assert (fr["frames"] == 1).all() and (fr["reserved"] == 0).all()
        assert (runs[0][1].view(np.uint8) == runs[1][1].view(np.uint8)).all()
        assert (runs[0][0] == runs[1][0]).all() and (runs[0][0] == runs[2][0]).all()
        a = runs[0][0].view(dabgpu.CIR_ACC_DTYPE).reshape(-1)
        want = frame_order_sum(fr, S, F, calls=2)
        assert (a["tap"].view(np.uint32) == want["tap"].view(np.uint32)).all()
        assert (a["carrier"].view(np.uint32) == want["carrier"].view(np.uint32)).all()
        assert (a["frames"] == 2 * F).all() and (a["reserved"] == 0).all()
        _, got = dabgpu.cir_analyse(a[0])
        assert [round(p["delay"]) for p in got] == [0, 23]


@pytest.mark.gpu
def test_gpu_recovered_channel_noiseless(cctx):
    """Paths (0, 1), (37, 0.5), (180, 0.25j) over 4 whole frames: exactly three paths, delays within 0.05 samples, levels
    -6.02 and -12.04 dB within 0.2 dB, nothing beyond the guard.  A fourth path at 600 is found within 0.5 samples,
    flagged BEYOND_GUARD, and the guard ratio is finite."""
    import torch
    ens = synth.Ensemble(seed=0xC12, n_frames=4)
    for paths, want in (([(0, 1.0), (37, 0.5), (180, 0.25j)], [(0, 0.0), (37, -6.0206), (180, -12.0412)]),
                        ([(0, 1.0), (37, 0.5), (180, 0.25j), (600, 0.5)], None)):
        x = synth.channel(ens.iq().ravel(), paths=paths)
        d = dev(torch, x)
        acc = cir_acc(torch, 1)
        zero = dev(torch, np.zeros(4, np.float32))
        cctx.cir_frames_dev(d.data_ptr() + NULL * 8, synth.NB_FRAME_SAMPLES, 1, 4, acc.data_ptr(), d_freq_offset=zero.data_ptr())
        cctx.sync()
        a = host(acc)[0]
        assert a["frames"] == 4
        rep, got = dabgpu.cir_analyse(a)
        got = paths_of(got)
        if want is not None:
            assert len(got) == 3, got
            for (dl, lv, _, beyond), (wd, wl) in zip(got, want):
                assert abs(dl - wd) <= 0.05 and abs(lv - wl) <= 0.2 and not beyond, got
            assert math.isinf(rep["guard_ratio_db"]) and rep["guard_ratio_db"] > 0
            assert rep["first_delay"] == got[0][0] and rep["strongest_delay"] == got[0][0] and rep["rms_delay_spread"] > 0
        else:
            far = [g for g in got if g[0] > 504]
            assert len(far) == 1 and abs(far[0][0] - 600) <= 0.5 and far[0][3], got
            assert all(not g[3] for g in got if g[0] < 504)
            assert [round(g[0]) for g in got if g[0] < 504] == [0, 37, 180]
            assert math.isfinite(rep["guard_ratio_db"])


@pytest.mark.gpu
def test_gpu_noise_floor(cctx):
    """10 dB SNR over 64 frames: the floor is within 10 % of the noise tap power the reference derives analytically."""
    import torch
    rng = np.random.default_rng(64)
    F = 64
    y = packed_prs(rng, [[(0, 1.0)]], F, SYM, snr_db=10.0)
    d = dev(torch, y)
    acc = cir_acc(torch, 1)
    zero = dev(torch, np.zeros(F, np.float32))
    cctx.cir_frames_dev(d.data_ptr(), SYM, 1, F, acc.data_ptr(), d_freq_offset=zero.data_ptr())
    cctx.sync()
    rep, got = dabgpu.cir_analyse(host(acc)[0])
    want = R.noise_tap_power(10 ** -1.0)
    assert abs(rep["floor"] / want - 1.0) < 0.10, (float(rep["floor"]), want)
    assert [round(g["delay"]) for g in got] == [0] and abs(rep["peak"] - 1.0) < 0.05


@pytest.mark.gpu
def test_gpu_sfn_cross_check_with_tii(cctx):
    """Three transmitters at delays 0 / 100 / 250, 0 / -3 / -6 dB: TII names all three and the CIR finds the three delays."""
    import torch
    ens = synth.Ensemble(seed=0x5F2, n_frames=4)
    tx = [(3, 10, 0, 0.0), (11, 45, 100, -3.0), (19, 62, 250, -6.0)]
    x = synth.sfn(np.tile(ens.frame_bits, (2, 1)), tx)
    x = synth.channel(x, snr_db=20.0, rng=np.random.default_rng(22))
    d = dev(torch, x)
    zero = dev(torch, np.zeros(8, np.float32))
    tacc = torch.zeros((1, 784), dtype=torch.uint8, device="cuda:0")
    cacc = cir_acc(torch, 1)
    cctx.tii_frames_dev(d.data_ptr() + NULL * 8, synth.NB_FRAME_SAMPLES, 1, 8, tacc.data_ptr(), d_freq_offset=zero.data_ptr())
    cctx.cir_frames_dev(d.data_ptr() + NULL * 8, synth.NB_FRAME_SAMPLES, 1, 8, cacc.data_ptr(), d_freq_offset=zero.data_ptr())
    cctx.sync()
    ids = dabgpu.tii_decode(tacc.cpu().numpy().view(dabgpu.TII_ACC_DTYPE).reshape(-1)[0])
    assert sorted((int(e["sub_id"]), int(e["main_id"])) for e in ids) == sorted((c, p) for c, p, _, _ in tx)
    rep, got = dabgpu.cir_analyse(host(cacc)[0])
    got = paths_of(got)
    assert len(got) == 3, got
    for (dl, lv, _, _), (_, _, wd, wl) in zip(got, tx):
        assert abs(dl - wd) <= 0.1 and abs(lv - wl) <= 0.3, got


@pytest.mark.gpu
def test_gpu_integer_formats_bit_exact(built):
    """cs16 / cs8 / cu8 records equal the cf32 records of the same values bit for bit (frequency array, even stride)."""
    import torch
    rng = np.random.default_rng(9)
    F, st = 6, SYM + 6
    y = packed_prs(rng, [[(0, 1.0), (17, 0.4)], None], F // 2, st, snr_db=12.0)
    y = np.concatenate([y, np.zeros(SYM, np.complex64)])
    fo = rng.uniform(-2, 2, F).astype(np.float32) / 2048
    v = np.stack([y.real, y.imag], -1).astype(np.float64)
    v /= np.sqrt((v ** 2).mean())
    c = make_ctx()
    try:
        for fmt, code, scale, dt, off in (("cs16", dabgpu.IQ_CS16, 2000.0, np.int16, 0.0), ("cs8", dabgpu.IQ_CS8, 25.0, np.int8, 0.0),
                                          ("cu8", dabgpu.IQ_CU8, 25.0, np.uint8, 127.5)):
            q = np.clip(np.round(v * scale + off), np.iinfo(dt).min, np.iinfo(dt).max).astype(dt)
            f = (q.astype(np.float32) - np.float32(off)).astype(np.float32)
            out = {}
            for name, fcode, arr in (("cf32", dabgpu.IQ_CF32, f), (fmt, code, q)):
                c.set_iq_format(fcode)
                d = dev(torch, arr)
                acc, frame = cir_acc(torch, 2), cir_acc(torch, F)
                d_fo = dev(torch, fo)
                c.cir_frames_dev(d.data_ptr(), st, 2, F // 2, acc.data_ptr(), d_freq_offset=d_fo.data_ptr(), d_frame=frame.data_ptr())
                c.sync()
                out[name] = (acc.cpu().numpy(), frame.cpu().numpy())
            assert (out["cf32"][0] == out[fmt][0]).all() and (out["cf32"][1] == out[fmt][1]).all(), fmt
            fr = out[fmt][1].view(dabgpu.CIR_ACC_DTYPE).reshape(-1)
            ref = R.records(f.view(np.complex64).ravel().astype(np.complex128), [i * st for i in range(F)], fo, budgets=True)
            close(fr, *ref)
    finally:
        c.set_iq_format(dabgpu.IQ_CF32)
        c.close()


@pytest.mark.gpu
def test_gpu_acquired_and_tracked_capture(cctx):
    """An unaligned capture of a two-path channel with an unknown carrier offset: acquire_dev, then track; cir_acquired_dev
    counts exactly the locked, whole frames, leaves the rest zero, matches the reference at each slot's start and offset,
    and recovers the paths' relative delay within 0.1 samples."""
    import torch
    L, MF = synth.NB_FRAME_SAMPLES, 6
    ens = synth.Ensemble(seed=0xA78, n_frames=4)
    bits = np.tile(ens.frame_bits, (3, 1))[:10]
    tx = np.concatenate([synth.modulate_frame(b) for b in bits])
    x = synth.channel(tx, snr_db=15.0, cfo=1.37 / 2048, paths=[(0, 1.0), (29, 0.6)], rng=np.random.default_rng(78))[70001:]
    d = dev(torch, x)
    n_cap, adv = 3 * L + 8192, 2 * L
    cctx.streams_reset(1)
    frames = torch.zeros((MF, 32), dtype=torch.uint8, device="cuda:0")
    counts = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    soft = torch.zeros((MF, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda:0")
    cctx.acquire_dev(d.data_ptr(), x.size, 1, n_cap, MF, frames.data_ptr(), counts.data_ptr())
    results = []
    for base, what in ((0, "acquire"), (adv, "track"), (2 * adv, "track")):
        if what == "track":
            cctx.ofdm_demod_tracked_dev(d.data_ptr() + base * 8, x.size, 1, n_cap, MF, adv, soft.data_ptr(), frames.data_ptr(),
                                        counts.data_ptr())
        acc, frame = cir_acc(torch, 1), cir_acc(torch, MF, fill=0x3C)
        cctx.cir_acquired_dev(d.data_ptr() + base * 8, x.size, 1, MF, frames.data_ptr(), acc.data_ptr(), timing_margin=64,
                              d_frame=frame.data_ptr())
        cctx.sync()
        fr = frames.cpu().numpy().view(dabgpu.ACQUIRED_FRAME_DTYPE).reshape(-1)
        results.append((what, base, fr.copy(), host(acc)[0].copy(), host(frame).copy()))
        if what == "acquire":
            cctx.track_start_dev(frames.data_ptr(), counts.data_ptr(), 1, MF, adv)
    for what, base, fr, a, rec in results:
        inside = (fr["flags"] == 3) & (fr["start"] + 64 >= 0)
        assert inside.sum() >= 2, (what, fr)
        assert a["frames"] == inside.sum() and (rec["frames"] == inside).all()
        assert (rec[~inside].view(np.uint8) == 0).all()
        sel = np.flatnonzero(inside)
        ref = R.records(x[base:].astype(np.complex128), fr["start"][sel] + 64, fr["freq_offset"][sel].astype(np.float64), budgets=True)
        close(rec[sel], *ref)
        _, got = dabgpu.cir_analyse(a)
        assert len(got) == 2, (what, paths_of(got))
        assert abs(float(got[1]["delay"] - got[0]["delay"]) - 29.0) <= 0.1, (what, paths_of(got))


@pytest.mark.gpu
def test_gpu_acquired_equals_aligned(cctx):
    """cir_acquired_dev on hand-built slots gives the records cir_frames_dev gives on the same frames, bit for bit; an
    unlocked slot, a slot that is not whole and one whose prefix lies before the capture give all-zero records."""
    import torch
    rng = np.random.default_rng(5)
    S, F = 2, 5
    y = packed_prs(rng, [[(0, 1.0), (44, 0.5j)], [(3, 0.8), (120, 0.6)]], F, SYM, snr_db=18.0)
    fo = (rng.uniform(-3.5, 3.5, S * F) / 2048).astype(np.float32)
    slots = np.zeros(S * F, dabgpu.ACQUIRED_FRAME_DTYPE)
    slots["start"] = np.tile(np.arange(F) * SYM - 64, S)
    slots["freq_offset"] = fo
    slots["flags"] = 3
    skipped = {3: 1, 6: 2, 8: 3}
    for i, fl in skipped.items():
        slots["flags"][i] = fl
    slots["start"][8] = -65                                  # prefix one sample before the capture
    d = dev(torch, y)
    d_fo = dev(torch, fo)
    d_slots = dev(torch, slots.view(np.uint8))
    a1, f1 = cir_acc(torch, S), cir_acc(torch, S * F)
    a2, f2 = cir_acc(torch, S), cir_acc(torch, S * F, fill=0x77)
    cctx.cir_frames_dev(d.data_ptr(), SYM, S, F, a1.data_ptr(), d_freq_offset=d_fo.data_ptr(), d_frame=f1.data_ptr())
    cctx.cir_acquired_dev(d.data_ptr(), F * SYM, S, F, d_slots.data_ptr(), a2.data_ptr(), timing_margin=64, d_frame=f2.data_ptr())
    cctx.sync()
    r1, r2 = host(f1), host(f2)
    for i in range(S * F):
        if i in skipped:
            assert (r2[i:i + 1].view(np.uint8) == 0).all(), i
        else:
            assert (r2[i:i + 1].view(np.uint8) == r1[i:i + 1].view(np.uint8)).all(), i
    assert list(host(a2)["frames"]) == [F - 1, F - 2]


@pytest.mark.gpu
def test_gpu_full_size_launch(built):
    """One launch of 16 384 frames: 64 streams x 256 PRS symbols packed at 2552 samples, each stream with its own channel.
    64 sampled frames match the reference; every stream's path list matches its truth."""
    import torch
    rng = np.random.default_rng(0xF011)
    S, F = 64, 256
    truth = []
    for s in range(S):
        n_extra = int(rng.integers(0, 3))
        delays = [0]
        while len(delays) < n_extra + 1:
            dd = int(rng.integers(8, 480))
            if all(abs(dd - e) >= 8 for e in delays):
                delays.append(dd)
        gains = [1.0] + [10 ** (-rng.uniform(1, 12) / 20) * np.exp(2j * np.pi * rng.uniform()) for _ in delays[1:]]
        truth.append(sorted(zip(delays, gains)))
    y = packed_prs(rng, truth, F, SYM, snr_db=20.0)
    c = make_ctx()
    try:
        d = dev(torch, y)
        del y
        zero = dev(torch, np.zeros(S * F, np.float32))
        acc, frame = cir_acc(torch, S), cir_acc(torch, S * F)
        c.cir_frames_dev(d.data_ptr(), SYM, S, F, acc.data_ptr(), d_freq_offset=zero.data_ptr(), d_frame=frame.data_ptr())
        c.sync()
        a = host(acc)
        assert (a["frames"] == F).all()
        pick = np.sort(rng.choice(S * F, 64, replace=False))
        rec = frame[torch.from_numpy(pick).to("cuda:0")].cpu().numpy().view(dabgpu.CIR_ACC_DTYPE).reshape(-1)
        for i, r in zip(pick, rec):
            w = d[i * SYM + 504:i * SYM + 2552].cpu().numpy().astype(np.complex128)
            close(r, *R.record(w, budgets=True))
        for s in range(S):
            _, got = dabgpu.cir_analyse(a[s])
            got = paths_of(got)
            want = truth[s]
            gmax = max(abs(g) for _, g in want)
            assert len(got) == len(want), (s, got, want)
            for (dl, lv, _, beyond), (wd, wg) in zip(got, want):
                assert abs(dl - wd) <= 0.1 and abs(lv - 20 * np.log10(abs(wg) / gmax)) <= 0.3 and not beyond, (s, got, want)
    finally:
        c.close()


@pytest.mark.gpu
def test_gpu_refusals_leave_outputs_untouched(built):
    import torch
    c = make_ctx()
    L = dabgpu.lib()
    try:
        d = dev(torch, np.zeros(8 * SYM, np.complex64))
        fo = dev(torch, np.zeros(8, np.float32))
        frames = torch.zeros((4, 32), dtype=torch.uint8, device="cuda:0")
        acc, frame = cir_acc(torch, 4, fill=0x5A), cir_acc(torch, 8, fill=0x5A)
        h, p, a, f = c._h, d.data_ptr(), acc.data_ptr(), frame.data_ptr()
        ERR_ARG, ERR_CAP = -1, -6
        cases = [
            (L.dabgpu_cir_frames_dev(None, p, SYM, 1, 2, fo.data_ptr(), f, a, None), ERR_ARG),
            (L.dabgpu_cir_frames_dev(h, None, SYM, 1, 2, fo.data_ptr(), f, a, None), ERR_ARG),
            (L.dabgpu_cir_frames_dev(h, p, SYM, 1, 2, fo.data_ptr(), f, None, None), ERR_ARG),
            (L.dabgpu_cir_frames_dev(h, p, SYM, -1, 2, fo.data_ptr(), f, a, None), ERR_ARG),
            (L.dabgpu_cir_frames_dev(h, p, SYM, 1, -2, fo.data_ptr(), f, a, None), ERR_ARG),
            (L.dabgpu_cir_frames_dev(h, p + 4, SYM, 1, 2, fo.data_ptr(), f, a, None), ERR_ARG),       # misaligned cf32
            (L.dabgpu_cir_frames_dev(h, p, SYM - 2, 1, 2, fo.data_ptr(), f, a, None), ERR_ARG),      # short stride
            (L.dabgpu_cir_frames_dev(h, p, SYM + 1, 1, 2, fo.data_ptr(), f, a, None), ERR_ARG),      # odd stride
            (L.dabgpu_cir_frames_dev(h, p, SYM, 1, 2, fo.data_ptr(), f, a + 2, None), ERR_ARG),      # misaligned acc
            (L.dabgpu_cir_frames_dev(h, p, SYM, 1, 2, fo.data_ptr(), f + 2, a, None), ERR_ARG),      # misaligned records
            (L.dabgpu_cir_frames_dev(h, p, SYM, 1, 2, None, f, a, None), ERR_ARG),                   # no stream states
            (L.dabgpu_cir_acquired_dev(None, p, SYM, 1, 4, frames.data_ptr(), 64, f, a, None), ERR_ARG),
            (L.dabgpu_cir_acquired_dev(h, None, SYM, 1, 4, frames.data_ptr(), 64, f, a, None), ERR_ARG),
            (L.dabgpu_cir_acquired_dev(h, p, SYM, 1, 0, frames.data_ptr(), 64, f, a, None), ERR_ARG),
            (L.dabgpu_cir_acquired_dev(h, p, SYM, 1, 4, None, 64, f, a, None), ERR_ARG),
            (L.dabgpu_cir_acquired_dev(h, p, SYM, 1, 4, frames.data_ptr(), -1, f, a, None), ERR_ARG),
            (L.dabgpu_cir_acquired_dev(h, p, SYM, 1, 4, frames.data_ptr(), 505, f, a, None), ERR_ARG),
            (L.dabgpu_cir_acquired_dev(h, p, SYM, 1, 4, frames.data_ptr(), 64, f, None, None), ERR_ARG),
            (L.dabgpu_cir_acquired_dev(h, p, SYM, 1, 4, frames.data_ptr() + 4, 64, f, a, None), ERR_ARG),  # misaligned slots
        ]
        c.streams_reset(1)
        cases.append((L.dabgpu_cir_frames_dev(h, p, SYM, 2, 2, None, f, a, None), ERR_CAP))     # more streams than states
        c.sync()
        assert [rc for rc, _ in cases] == [want for _, want in cases]
        assert (acc.cpu().numpy() == 0x5A).all() and (frame.cpu().numpy() == 0x5A).all()
        # zero frames: OK, nothing written; one frame: any stride
        assert L.dabgpu_cir_frames_dev(h, p, SYM, 0, 2, None, f, a, None) == 0
        c.sync()
        assert (acc.cpu().numpy() == 0x5A).all()
        assert L.dabgpu_cir_frames_dev(h, p, 1, 1, 1, fo.data_ptr(), f, a, None) == 0
        c.sync()
        assert host(frame)[0]["frames"] == 1 and (frame.cpu().numpy()[1:] == 0x5A).all()
    finally:
        c.close()
