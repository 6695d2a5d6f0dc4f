"""The front end's run queue: a launch has at most as many wavefronts as the device holds at once, each starts on
the item of its own number and takes every further one from a device counter; the counter pair is handed back zeroed by the
launch's last wave.  That can only go wrong where a wave takes a second run, where two launches are in flight, or where a
launch is smaller than the grid -- the shapes below.  Bars: soft bits within one int8 LSB of the oracle and correlations within
1e-3 of the frame's largest (tests/test_gpu_parity.py); whatever cut a context is given, the bytes are the default plan's.

96 frames cut into 75 runs each are 7 200 one-symbol runs for the 3 072 resident waves of an MI355X: every wave takes two or
three.  24 frames (1 800 runs) stay below the grid, 48 (3 600) go past it again."""
import numpy as np
import pytest

import dabgpu
from conftest import make_ctx
from dabgpu import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SOFT_TOL = 1             # int8 LSB
CYC_TOL = 1e-3           # of the frame's largest correlation
SYMS = 76 * 2552
N_REUSE = 96
SENTINEL = -128          # no soft bit has this value (they are in -127..127)


def quantise(x, fmt):
    """complex64 samples -> (integer samples [..., 2] of format `fmt`, the float32 complex values they stand for: cu8 is u - 127.5)"""
    v = np.stack([x.real, x.imag], axis=-1).astype(np.float64)
    v *= {"cs16": 2000.0, "cu8": 25.0}[fmt] / float(np.sqrt(np.mean(v * v)))
    if fmt == "cs16":
        q = np.clip(np.rint(v), -32768, 32767).astype(np.int16)
        f = q.astype(np.float32)
    else:
        q = np.clip(np.rint(v + 127.5), 0, 255).astype(np.uint8)
        f = q.astype(np.float32) - np.float32(127.5)
    return q, np.ascontiguousarray(f).view(np.complex64)[..., 0]


def freq_offsets(n):
    """a different correction per frame, around the channel's -0.3 carriers"""
    return ((-0.3 + 0.004 * np.arange(n)) / 2048).astype(np.float32)


@pytest.fixture(scope="module")
def base_frames(built, ensemble_iq):
    """five PRS-aligned received frames (14 dB, 0.3 carriers off)"""
    rng = np.random.default_rng(23)
    rx = synth.channel(ensemble_iq.ravel(), snr_db=14.0, cfo=0.3 / 2048, rng=rng).reshape(ensemble_iq.shape)
    return np.ascontiguousarray(rx[:, synth.NB_NULL:synth.NB_NULL + SYMS])


@pytest.fixture(scope="module")
def oracle_of(base_frames):
    """frame f of a batch is base frame f % 5 corrected by freq_offsets()[f]: its oracle outputs, computed once"""
    cache = {}

    def get(f, fo):
        key = (f % base_frames.shape[0], float(fo))
        if key not in cache:
            soft, _, cyc, _ = O.ofdm_demod_frame(base_frames[key[0]], key[1], want_cyc=True)
            cache[key] = (soft, cyc)
        return cache[key]
    return get


def batch(base, n, dev):
    import torch
    t = torch.from_numpy(base).to(dev)
    return t.repeat((n + t.shape[0] - 1) // t.shape[0], *([1] * (t.dim() - 1)))[:n].contiguous()


def demod(ctx, iq, stride, n, fo, want_cyc=True, stream=None):
    """one device-pointer call on buffers filled with a sentinel first -> (soft, cyc) tensors"""
    import torch
    soft = torch.full((n, dabgpu.NB_FRAME_BITS), SENTINEL, dtype=torch.int8, device=iq.device)
    cyc = torch.full((n, 76, 2), float("nan"), dtype=torch.float32, device=iq.device) if want_cyc else None
    ctx.ofdm_demod_frames_dev(iq.data_ptr(), stride, n, fo.data_ptr(), soft.data_ptr(), cyc.data_ptr() if want_cyc else None, None,
                              stream)
    return soft, cyc


def check_against_oracle(soft, cyc, fo, oracle_of):
    soft, cyc = soft.cpu().numpy(), (cyc.cpu().numpy().view(np.complex64)[..., 0] if cyc is not None else None)
    for f in range(soft.shape[0]):
        osoft, ocyc = oracle_of(f, fo[f])
        worst = int(np.abs(soft[f].astype(np.int32) - osoft.astype(np.int32)).max())
        assert worst <= SOFT_TOL, (f, worst)
        if cyc is not None:
            assert np.abs(cyc[f] - ocyc).max() <= CYC_TOL * np.abs(ocyc).max(), f


def test_every_wave_takes_a_second_run(base_frames, oracle_of):
    """96 frames in 7 200 one-symbol runs, correlations out, a different frequency correction per frame"""
    import torch
    dev = torch.device("cuda", 0)
    iq = batch(base_frames.view(np.float32).reshape(-1, SYMS, 2), N_REUSE, dev)
    fo_h = freq_offsets(N_REUSE)
    fo = torch.from_numpy(fo_h).to(dev)
    outs = []
    for runs in (75, 0):
        c = make_ctx(None, N_REUSE, ofdm_symbol_runs=runs)
        try:
            soft, cyc = demod(c, iq, SYMS, N_REUSE, fo)
            c.sync()
            outs.append((soft, cyc))
        finally:
            c.close()
    check_against_oracle(outs[0][0], outs[0][1], fo_h, oracle_of)
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))


@pytest.mark.parametrize("n", [24, 48])
@pytest.mark.parametrize("fmt", ["cs16", "cu8"])
def test_runs_reused_on_integer_samples(base_frames, fmt, n):
    """the same cut on cs16 and cu8 samples: 24 frames (fewer runs than waves) and 48 (more)"""
    import torch
    dev = torch.device("cuda", 0)
    q, as_float = quantise(base_frames, fmt)
    iq = batch(q, n, dev)
    fo_h = freq_offsets(n)
    fo = torch.from_numpy(fo_h).to(dev)
    outs = []
    for runs in (75, 0):
        c = make_ctx(None, n, ofdm_symbol_runs=runs)
        try:
            c.set_iq_format({"cs16": dabgpu.IQ_CS16, "cu8": dabgpu.IQ_CU8}[fmt])
            soft, cyc = demod(c, iq, SYMS, n, fo)
            c.sync()
            outs.append((soft, cyc))
        finally:
            c.close()
    soft, cyc = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy().view(np.complex64)[..., 0]
    for f in range(n):
        k = f % as_float.shape[0]
        osoft, _, ocyc, _ = O.ofdm_demod_frame(as_float[k], float(fo_h[f]), want_cyc=True)
        assert np.abs(soft[f].astype(np.int32) - osoft.astype(np.int32)).max() <= SOFT_TOL, f
        assert np.abs(cyc[f] - ocyc).max() <= CYC_TOL * np.abs(ocyc).max(), f
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))


@pytest.mark.parametrize("n", [1, 3, 5])
def test_launches_smaller_than_the_grid(base_frames, oracle_of, n):
    """the default plan on 1, 3 and 5 frames: fewer items than resident waves, a last workgroup that is not full"""
    import torch
    dev = torch.device("cuda", 0)
    iq = batch(base_frames.view(np.float32).reshape(-1, SYMS, 2), n, dev)
    fo_h = freq_offsets(n)
    fo = torch.from_numpy(fo_h).to(dev)
    c = make_ctx(None, 8)
    try:
        soft, cyc = demod(c, iq, SYMS, n, fo)
        c.sync()
    finally:
        c.close()
    check_against_oracle(soft, cyc, fo_h, oracle_of)


def test_counter_pairs_come_back_zeroed(base_frames):
    """300 calls in a row on each of two contexts, each on a stream of its own, in one loop: more calls than a ring has
    pairs, alternating between 5 and 96 frames of 75 runs each; every call writes what the first call of its shape wrote"""
    import torch
    dev = torch.device("cuda", 0)
    iq = batch(base_frames.view(np.float32).reshape(-1, SYMS, 2), N_REUSE, dev)
    fo = torch.from_numpy(freq_offsets(N_REUSE)).to(dev)
    shapes = (5, N_REUSE)
    ctxs = [make_ctx(None, N_REUSE, ofdm_symbol_runs=75) for _ in range(2)]
    streams = [torch.cuda.Stream(device=dev) for _ in ctxs]
    try:
        first = [{} for _ in ctxs]
        bad = [torch.zeros((), dtype=torch.int32, device=dev) for _ in ctxs]
        torch.cuda.synchronize()                           # (what was made above on torch's stream is used on two others)
        for call in range(300):
            n = shapes[call & 1]
            for k, (c, st) in enumerate(zip(ctxs, streams)):
                with torch.cuda.stream(st):
                    soft, cyc = demod(c, iq, SYMS, n, fo, stream=st.cuda_stream)
                    if n not in first[k]:
                        first[k][n] = (soft, cyc)
                    else:
                        bad[k] += (soft != first[k][n][0]).any().to(torch.int32)
                        bad[k] += (cyc.view(torch.int32) != first[k][n][1].view(torch.int32)).any().to(torch.int32)
        torch.cuda.synchronize()
        for k in range(len(ctxs)):
            assert int(bad[k]) == 0, (k, int(bad[k]))
            for n in shapes:
                assert not bool((first[k][n][0] == SENTINEL).any())
            # ... and the two contexts, given the same samples, agree with each other
            for n in shapes:
                assert torch.equal(first[k][n][0], first[0][n][0])
    finally:
        for c in ctxs:
            c.close()


def test_mover_writes_every_soft_byte(base_frames):
    """the geometry mover on the same 7 200 runs: what it writes does not depend on what the buffer held, so no byte is left out"""
    import torch
    dev = torch.device("cuda", 0)
    iq = batch(base_frames.view(np.float32).reshape(-1, SYMS, 2), N_REUSE, dev)
    c = make_ctx(None, N_REUSE, ofdm_symbol_runs=75)
    try:
        outs = []
        for sentinel in (0x55, -0x56):
            soft = torch.full((N_REUSE, dabgpu.NB_FRAME_BITS), sentinel, dtype=torch.int8, device=dev)
            c.mover_frames_dev(iq.data_ptr(), SYMS, N_REUSE, soft.data_ptr(), True)
            c.sync()
            outs.append(soft)
        assert torch.equal(outs[0], outs[1])
    finally:
        c.close()
