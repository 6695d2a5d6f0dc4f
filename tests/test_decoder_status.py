"""The decoder half of the C ABI checks a sub-channel list in one place (csrc/decode_plan.hpp, SubchannelPlan) and keeps
the de-interleaver rings of its two state-keeping calls in one type (csrc/dabgpu_ctx.hpp, HistoryRings).  What a caller
sees of both: the status of a call that is wrong in exactly one way, on every entry point that takes a list; that a
refused call leaves the kept rings alone; the life of a ring through both of its owners.

The expected codes are literals, recorded from the library before the entry points shared their validation: every
single-fault row returns what it returned then.

Not in the table: a length no decoder holds (DABGPU_ERR_CAPACITY out of lookup_code).  No valid descriptor reaches it:
every DAB bit rate is a multiple of 8 kbit/s, so nsteps = 24 * bitrate + 6 always has whole phase cycles and whole
32-bit output words, which is all dabk::lane_supported asks for, up to the 1824 kbit/s that fit into 864 capacity units.

Asserted elsewhere, not again here: dabgpu_decode_stream_reset followed by a call equals a fresh start
(test_streams.py::test_stream_decoder_keeps_the_deinterleaver_state), dabgpu_pipe_reset likewise
(test_pipeline.py::test_ring_equals_the_synchronous_calls).  dabgpu_test_fail_frame_call reaches the one-frame calls
only, so the failed-call check runs through dabgpu_decode_stream_frames and not through the ring."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth
from conftest import ROOT, make_ctx

ARG, HIP, PROFILE = -1, -2, -5
L = dabgpu.FRAME_USED_SAMPLES
N_FRAMES = 7            # the 5-frame multiplex tiled: 28 CIFs, enough for a ring restarted at CIF 8 to fill again (15 CIFs)

ENTRY_POINTS = ["msc_decode_multi_dev", "decode_frames_dev", "decode_frames", "decode_stream_frames_quality", "channel_ber_dev",
                "pipe_submit"]


def _a(ens):
    return dabgpu.subchannel(ens.start_cu, 64, level=3)                 # the multiplex's sub-channel: 48 CUs from 0


def _b(start=100):
    return dabgpu.subchannel(start, 32, level=2)                        # 32 CUs of the random filler


def _faults(ens):
    """name -> (list, index of the output pointer to null or None, pass a null list, expected status)"""
    a, b = _a(ens), _b()
    return {
        "bad protection level": ([a, dabgpu.Subchannel(100, 32, 0, 0, 9, 32)], None, False, PROFILE),
        "length not the profile's": ([a, dabgpu.Subchannel(100, 31, 0, 0, 2, 32)], None, False, PROFILE),
        "start + length > 864": ([a, _b(840)], None, False, ARG),
        "negative start": ([a, _b(-1)], None, False, ARG),
        "two overlapping entries": ([a, _b(40)], None, False, ARG),
        "the same entry twice": ([a, a], None, False, ARG),
        "null out[1]": ([a, b], 1, False, ARG),
        "null list, n = 2": ([a, b], None, True, ARG),
    }


class Rig:
    """one frame's buffers for every entry point, on one context with an open ring"""

    def __init__(self, c, frames, fo):
        import torch
        self.c, self.lib, self.h = c, c._lib, c._h
        dev = torch.device("cuda", 0)
        self.frames, self.fo = frames, fo
        self.soft = np.ascontiguousarray(c.ofdm_demod_frames(frames, fo)[0])
        self.d_soft = torch.from_numpy(self.soft[:1]).to(dev)
        self.d_fib = torch.zeros((12, 32), dtype=torch.uint8, device=dev)
        self.d_ok = torch.zeros(12, dtype=torch.uint8, device=dev)
        self.d_out = [torch.zeros((4, 192), dtype=torch.uint8, device=dev) for _ in range(3)]
        self.d_ber = [torch.zeros((4, 2), dtype=torch.int32, device=dev) for _ in range(3)]
        self.fib, self.ok = np.zeros((12, 32), np.uint8), np.zeros(12, np.uint8)
        self.out = [np.zeros((4, 192), np.uint8) for _ in range(3)]
        torch.cuda.synchronize()
        c.pipe_open(2, 1, L)

    def call(self, entry, scs, null_out=None, null_list=False, ber_offset=0, frame=0):
        """-> status of `entry` on one frame with the list `scs`"""
        n = len(scs)
        arr = None if null_list else (dabgpu.Subchannel * n)(*scs)

        def ptrs(addresses):
            return (C.c_void_p * n)(*[None if i == null_out else x for i, x in enumerate(addresses[:n])])
        host, device = ptrs([o.ctypes.data for o in self.out]), ptrs([t.data_ptr() for t in self.d_out])
        soft, stride = self.soft[frame:frame + 1], dabgpu.NB_FRAME_BITS
        lib, h, p = self.lib, self.h, dabgpu._p
        if entry == "msc_decode_multi_dev":
            return lib.dabgpu_msc_decode_multi_dev(h, arr, n, self.d_soft.data_ptr(), stride, 1, 1, None, None, device, None)
        if entry == "decode_frames_dev":
            return lib.dabgpu_decode_frames_dev(h, self.d_soft.data_ptr(), stride, 1, 1, self.d_fib.data_ptr(), self.d_ok.data_ptr(),
                                                arr, n, None, None, device, None)
        if entry == "decode_frames":
            return lib.dabgpu_decode_frames(h, p(soft), stride, 1, 1, p(self.fib), p(self.ok), arr, n, None, None, host)
        if entry == "decode_stream_frames_quality":
            return lib.dabgpu_decode_stream_frames_quality(h, p(soft), stride, 1, p(self.fib), p(self.ok), arr, n, host, None, None, None)
        if entry == "channel_ber_dev":
            counts = (C.c_void_p * n)(*[t.data_ptr() + (ber_offset if i == 1 else 0) for i, t in enumerate(self.d_ber[:n])])
            return lib.dabgpu_channel_ber_dev(h, self.d_soft.data_ptr(), stride, 1, 1, None, None, arr, n, None, device, counts, None)
        assert entry == "pipe_submit"
        t = C.c_int64(-1)
        rc = lib.dabgpu_pipe_submit(h, self.frames[frame:frame + 1].ctypes.data, 1, 1, self.fo[frame:frame + 1].ctypes.data, 0.9, arr, n,
                                    None, p(self.fib), p(self.ok), host, C.byref(t))
        if rc == 0:
            assert lib.dabgpu_pipe_wait(h, t.value) == 0
        return rc

    def close(self):
        self.c.sync()
        self.c.pipe_close()
        self.c.close()


@pytest.fixture(scope="module")
def stream(ensemble, ensemble_iq):
    """N_FRAMES consecutive frames from the PRS on, their offsets"""
    tx = np.tile(ensemble_iq, (2, 1))[:N_FRAMES]
    rx = synth.channel(tx.ravel(), snr_db=16.0, cfo=0.0, rng=np.random.default_rng(11)).reshape(tx.shape)
    return np.ascontiguousarray(rx[:, synth.NB_NULL:synth.NB_NULL + L]), np.zeros(N_FRAMES, np.float32)


@pytest.fixture(scope="module")
def rig(built, stream):
    r = Rig(make_ctx(None, 8), *stream)
    yield r
    r.close()


@pytest.fixture(scope="module")
def reference(rig, ensemble):
    """[a, b] decoded in one go over the whole stream, and as if the stream began at frame 2: ([out_a, out_b], [late_a, late_b]),
    each [CIFs][bytes]"""
    scs = [_a(ensemble), _b()]
    whole = [o[0] for o in rig.c.decode_frames(rig.soft, 1, scs)[2]]
    late = [o[0] for o in rig.c.decode_frames(rig.soft[2:], 1, scs)[2]]
    for t in range(15, 4 * N_FRAMES):                                    # the transmitter's bytes, once the de-interleaver has filled
        assert (whole[0][t] == ensemble.msc_bytes[(t - 15) % (4 * ensemble.n_frames)]).all(), t
    return whole, late


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_single_fault_status(rig, ensemble, entry):
    a, b = _a(ensemble), _b()
    assert rig.call(entry, [a, b]) == 0
    faults = _faults(ensemble)
    got = {name: rig.call(entry, scs, null_out, null_list) for name, (scs, null_out, null_list, _) in faults.items()}
    want = {name: row[3] for name, row in faults.items()}
    if entry == "channel_ber_dev":
        got["misaligned count pointer"], want["misaligned count pointer"] = rig.call(entry, [a, b], ber_offset=4), ARG
    # wrong in two ways -- an earlier overlap and a later bad descriptor: dabgpu.h promises no precedence, either code is right
    both = rig.call(entry, [a, _b(40), dabgpu.Subchannel(200, 32, 0, 0, 9, 32)])
    for name in got:
        print(entry, "|", name, "->", got[name])
    print(entry, "| overlap, then a bad protection level ->", both)
    assert got == want
    assert both in (ARG, PROFILE)
    assert rig.call(entry, [a, b]) == 0
    rig.c.sync()
    rig.c.decode_stream_reset()
    rig.c.pipe_reset()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["decode_stream_frames_quality", "pipe_submit"])
def test_refused_calls_leave_the_rings_alone(rig, ensemble, reference, entry):
    """Two frames, every refused row of the table on the third, then the third and two more: the bytes of all five equal the
    uninterrupted decode (and so the transmitter's from CIF 15 on) -- no ring was flipped, dropped or re-made by a refusal."""
    scs = [_a(ensemble), _b()]
    rig.c.decode_stream_reset()
    rig.c.pipe_reset()
    got = [[], []]

    def good(f):
        assert rig.call(entry, scs, frame=f) == 0
        for k in range(2):
            nb = scs[k].bitrate_kbps * 3                                 # (the library packs [4][nb] into the buffer's front)
            got[k].append(rig.out[k].ravel()[:4 * nb].reshape(4, nb).copy())
    good(0)
    good(1)
    for name, (bad, null_out, null_list, want) in _faults(ensemble).items():
        assert rig.call(entry, bad, null_out, null_list, frame=2) == want, name
    for f in (2, 3, 4):
        good(f)
    for k in range(2):
        assert (np.concatenate(got[k]) == reference[0][k][:20]).all(), k
    rig.c.decode_stream_reset()
    rig.c.pipe_reset()


def _decode(c, owner, rig, f, scs):
    """frame f of the stream through one of the two ring owners -> [out_i [4][bytes]]"""
    if owner == "stream":
        return [o[0] for o in c.decode_stream_frames(rig.soft[f:f + 1], scs)[2]]
    fib, ok = np.zeros((1, 12, 32), np.uint8), np.zeros((1, 12), np.uint8)
    outs = [np.zeros((4, sc.bitrate_kbps * 3), np.uint8) for sc in scs]
    c.pipe_wait(c.pipe_submit(rig.frames[f:f + 1], 1, 1, rig.fo[f:f + 1], scs, None, fib, ok, outs))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("owner", ["stream", "pipe"])
def test_ring_lifecycle(ctx, rig, ensemble, reference, owner):
    """One frame per call (15 CIFs take four frames, hence seven calls), two sub-channels, through both kernel selections.
    A sub-channel left out of one call comes back from erasures: its bytes equal a stream that began there, differ from
    the uninterrupted decode while its ring fills (15 CIFs) and equal it afterwards; the other sub-channel never notices.
    A call that fails part-way (the test hook) drops every ring: all sub-channels continue as a stream that began there."""
    a, b = _a(ensemble), _b()
    whole, late = reference
    ctx.decode_stream_reset()
    if owner == "pipe":
        ctx.pipe_open(2, 1, L)
    try:
        out_a, out_b = [], []
        for f in range(N_FRAMES):
            outs = _decode(ctx, owner, rig, f, [a] if f == 1 else [a, b])
            out_a.append(outs[0])
            if f >= 2:
                out_b.append(outs[1])
        out_a, out_b = np.concatenate(out_a), np.concatenate(out_b)
        assert (out_a == whole[0]).all()
        assert (out_b == late[1]).all()                                   # b: CIFs 8 .. 27 of the stream
        assert (out_b[0] != whole[1][8]).any() and (out_b[:15] != whole[1][8:23]).any()
        assert (out_b[15:] == whole[1][23:]).all()
        if owner == "stream":
            ctx.decode_stream_reset()
            for f in (0, 1):
                _decode(ctx, owner, rig, f, [a, b])
            ctx.test_fail_frame_call(1)
            with pytest.raises(dabgpu.DabGpuError) as e:
                _decode(ctx, owner, rig, 2, [a, b])
            assert e.value.status == HIP
            for f in (2, 3):
                outs = _decode(ctx, owner, rig, f, [a, b])
                for k in range(2):
                    assert (outs[k] == late[k][4 * (f - 2):4 * (f - 1)]).all(), (f, k)
                    assert (outs[k] != whole[k][4 * f:4 * f + 4]).any(), (f, k)
    finally:
        if owner == "pipe":
            ctx.pipe_close()
        ctx.decode_stream_reset()


# ---------------------------------------------------------------------------------------------- without a GPU
#: `nm -D --defined-only libdabgpu.so`, the dabgpu_* names: what the library exported before the decoder's entry points were
#: regrouped (dabgpu_mer_dev and dabgpu_channel_ber_dev changed translation unit) -- nothing added, nothing removed
EXPORTED = sorted(dabgpu.EXPORTS)


def test_exported_names_are_unchanged(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", dabgpu.LIB_PATH], text=True)
    names = sorted(line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("dabgpu_"))
    assert names == EXPORTED


def test_fake_abi_compiles_against_the_header():
    """tests/fake_abi implements every entry point the host mirror uses with the header's own prototypes: a changed
    signature in include/dabgpu.h is a compile error here"""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(ROOT, "tests", "fake_abi"),
           "-I" + os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")]
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only"] + inc + [os.path.join(ROOT, "tests", "fake_abi", "fake_dabgpu.cpp")])
