"""ETI(NI) to IQ (include/dabgpu.h, "ETI(NI) to IQ"): the device modulator held to tests/modulator_reference.py -- the
transmitted signal composed from dabgpu.synth -- sample by sample, bit by bit through the library's own front end, and
byte by byte through the whole receive chain back to ETI.

The ensemble is the smallest that reaches every branch: 5 transmission frames (20 CIFs: past the interleaver's 15 and across
frame boundaries), an EEP-A sub-channel whose 24 CUs from CU 40 straddle the OFDM symbol boundary at CU 48, an EEP-B one,
a UEP one from a table row with padding bits (index 4), unallocated CUs before, between and behind them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dabgpu
import eti_reference as E
import modulator_reference as M
from conftest import ROOT, make_ctx
from dabgpu import synth

CSRC = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "csrc")
N_FRAMES, N_CIF = 5, 20
REF = [{"id": 9, "start": 70, "bitrate": 32, "uep": False, "eep_type": 1, "level": 2},     # EEP 2-B, 21 CUs
       {"id": 2, "start": 100, "bitrate": 32, "uep": True, "eep_type": 0, "level": 1},     # UEP index 4, 35 CUs, 4 padding bits
       {"id": 5, "start": 40, "bitrate": 32, "uep": False, "eep_type": 0, "level": 3}]     # EEP 3-A, 24 CUs
# |device - reference| over the frame's peak magnitude: the bound test_fft_stage_matches_oracle_and_numpy holds the forward FFT to
IQ_BOUND = 1e-4


def streams():
    """The list eti_layout takes, in an order that is not the frame's."""
    return [(9, dabgpu.subchannel(70, 32, level=2, eep_type=1)), (2, dabgpu.uep_subchannel(4, 100)),
            (5, dabgpu.subchannel(40, 32, level=3))]


def contents(seed):
    rng = np.random.default_rng(seed)
    fibs = synth.make_fibs(rng, 3 * N_CIF).reshape(N_CIF, 3, 32)
    data = {st["id"]: rng.integers(0, 256, (N_CIF, st["bitrate"] * 3), dtype=np.uint8) for st in REF}
    return fibs, data


@pytest.fixture(scope="module")
def case():
    """Stream 0's contents, its ETI frames, the reference's frame bits and IQ (computed once, never modified)."""
    fibs, data = contents(100)
    eti = M.build_eti(REF, fibs, data)
    bits = M.frame_bits(REF, fibs, data)
    iq = M.modulate(bits)
    for a in (fibs, eti, bits, iq):
        a.setflags(write=False)
    return {"fibs": fibs, "data": data, "eti": eti, "bits": bits, "iq": iq}


def worst_over_peak(got, want):
    """max |got - want| / max |want| per frame -> the worst frame's."""
    got, want = np.asarray(got).reshape(len(want), -1), np.asarray(want)
    return max(float(np.abs(got[f].astype(np.complex128) - want[f]).max() / np.abs(want[f]).max()) for f in range(len(want)))


# ------------------------------------------------------------------ CPU
def test_stream_list_round_trip(built, case):
    sts = streams()
    plan = dabgpu.eti_layout(sts)
    got = dabgpu.eti_streams(case["eti"][7])
    assert len(got) == 3
    for k, g in enumerate(got):
        scid, sc = sts[plan.order[k]]
        assert g.subchannel_id == scid
        assert [getattr(g.sc, f) for f, _ in dabgpu.Subchannel._fields_] == [getattr(sc, f) for f, _ in dabgpu.Subchannel._fields_]
    again = dabgpu.eti_layout(got)
    assert bytes(again.header) == bytes(plan.header) and list(again.order[:3]) == [0, 1, 2]
    assert [g.sc.start_address for g in got] == [40, 70, 100] and [g.sc.length for g in got] == [24, 21, 35]
    # TPL/STL pairs that name no profile: EEP-B at 48 kbit/s (not a multiple of 32), UEP 320 kbit/s at level 3 (no such row),
    # EEP option 2, a bit rate that is not a multiple of 8 (STL 5)
    for bad in ({"id": 1, "start": 0, "bitrate": 48, "uep": False, "eep_type": 1, "level": 2},
                {"id": 1, "start": 0, "bitrate": 320, "uep": True, "eep_type": 0, "level": 3},
                {"id": 1, "start": 0, "bitrate": 32, "uep": False, "eep_type": 2, "level": 2}):
        frame = E.write_frame([bad], 0, bytes(96), {1: bytes(bad["bitrate"] * 3)}, 0xFF)
        with pytest.raises(dabgpu.DabGpuError) as e:
            dabgpu.eti_streams(frame)
        assert e.value.status == -1
    frame = bytearray(E.write_frame([REF[2]], 0, bytes(96), {5: bytes(96)}, 0xFF))
    frame[11] = 5
    with pytest.raises(dabgpu.DabGpuError):
        dabgpu.eti_streams(bytes(frame))
    assert dabgpu.eti_streams(E.write_frame([], 0, bytes(96), {}, 0xFF)) == []


def test_reference_decodes_through_the_oracle(built, case):
    """The reference's own IQ, through the CPU oracle's front end, FIC and MSC decoders, gives back the FIBs of every CIF and
    the stream bytes of every logical frame whose 16 CIFs lie inside the signal (CIFs 15 and later)."""
    from oracle import oracle as O
    soft = np.stack([O.ofdm_demod_frame(case["iq"][f][synth.NB_NULL:], 0.0)[0] for f in range(N_FRAMES)])
    assert ((soft > 0).astype(np.uint8) == case["bits"]).all()
    for f in range(N_FRAMES):
        fib, ok = O.fic_decode(soft[f])
        assert ok.all() and (fib.reshape(4, 3, 32) == case["fibs"][4 * f:4 * f + 4]).all()
    cifs = soft[:, synth.NB_FIC_BITS:].reshape(N_CIF, synth.NB_CIF_BITS)
    for st in REF:
        mask, size_cu = M.mask_of(st)
        a = 64 * st["start"]
        for t in range(15, N_CIF):
            de = O.time_deinterleave(cifs[t - 15:t + 1, a:a + 64 * size_cu])
            got = O.msc_decode_lf(de[:int(mask.sum())], mask, st["bitrate"] * 24 + 6)
            assert (got == case["data"][st["id"]][t - 15]).all(), (st["id"], t)


def test_modulator_kernels_use_no_scratch_and_spill_nothing(built):
    from test_device_asm import kernel_metadata
    obj = os.path.join(CSRC, "mod_kernels.o")
    tools = "/opt/rocm/lib/llvm/bin/"
    if not os.path.exists(obj):
        subprocess.check_call(["make", "-C", CSRC, "mod_kernels.o"], stdout=subprocess.DEVNULL)
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "mod.fat"), os.path.join(td, "mod.co")
        subprocess.check_call([tools + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([tools + "clang-offload-bundler", "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + fat, "--output=" + co])
        md = kernel_metadata(subprocess.check_output([tools + "llvm-readelf", "--notes", co], text=True))
    assert sorted(k.split("mod_")[1].split("_kernel")[0] for k in md) == ["encode", "phase", "symbol", "tii"], list(md)
    for k, v in md.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v.get("agpr_count", 0) == 0 and v["vgpr_count"] <= 64, (k, v)               # 8 waves per SIMD
    sym = [v for k, v in md.items() if "mod_symbol_kernel" in k][0]
    assert sym["group_segment_fixed_size"] <= 160 * 1024 // 4                             # four symbols in flight per CU


def test_refusals_that_need_no_device(built):
    """Every argument check comes before the context is used: a stand-in context (zeroed memory) is enough to see them."""
    L = dabgpu.lib()
    sts = streams()
    plan = dabgpu.eti_layout(sts)
    arr = (dabgpu.EtiStream * 3)(*[dabgpu.EtiStream(i, sc) for i, sc in sts])
    fake = C.create_string_buffer(1 << 16)
    A = 1 << 20                                                  # any 16-byte aligned address: nothing is dereferenced

    def call(**kw):
        a = dict(ctx=C.addressof(fake), plan=plan, streams=arr, cfg=None, n_streams=0, fps=0, eti=A, sin=None, sout=None, iq=A,
                 stride=196608, status=A)
        a.update(kw)
        return L.dabgpu_modulate_eti_dev(a["ctx"], C.byref(a["plan"]), a["streams"], a["cfg"], a["n_streams"], a["fps"], a["eti"],
                                         a["sin"], a["sout"], a["iq"], a["stride"], a["status"], None)
    assert call() == 0                                           # nothing to do: accepted, nothing enqueued
    assert call(ctx=None) == -1 and call(eti=None) == -1 and call(iq=None) == -1 and call(status=None) == -1
    assert call(n_streams=-1) == -1 and call(fps=-1) == -1
    assert call(stride=196607) == -1 and call(stride=196609) == -1 and call(stride=196610) == 0
    assert call(iq=A + 8) == -1 and call(eti=A + 4) == -1 and call(status=A + 4) == -1 and call(sin=A + 8) == -1
    assert call(sin=A, sout=A) == -1 and call(sin=A, sout=A + (1 << 18)) == 0
    assert call(cfg=C.byref(dabgpu.mod_cfg(tii_main=70, tii_sub=0))) == -1 and call(cfg=C.byref(dabgpu.mod_cfg(tii_main=3))) == -1
    assert call(cfg=C.byref(dabgpu.mod_cfg(tii_main=69, tii_sub=23))) == 0 and call(cfg=C.byref(dabgpu.mod_cfg(tii_sub=24, tii_main=0))) == -1
    bad = dabgpu.eti_layout(sts)
    bad.bytes[1] = 100
    assert call(plan=bad) == -1
    bad = dabgpu.eti_layout(sts)
    bad.order[0] = 3
    assert call(plan=bad) == -1
    # a sub-channel whose size is not its profile's
    wrong = (dabgpu.EtiStream * 3)(*[dabgpu.EtiStream(i, sc) for i, sc in sts])
    wrong[2].sc.length = 23
    assert call(streams=wrong) == -5
    cfg = dabgpu.mod_cfg()
    assert (cfg.gain, cfg.tii_main, cfg.tii_sub, cfg.reserved) == (1.0, -1, -1, 0)
    assert dabgpu.mod_state_bytes() == 15 * 6912


def test_struct_layouts_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dabgpu.h"', 'int main(void) {',
             '  printf("%zu %zu %zu\\n", sizeof(dabgpu_mod_status), offsetof(dabgpu_mod_status, flags), offsetof(dabgpu_mod_status, refused));',
             '  printf("%zu %zu %zu %zu\\n", sizeof(dabgpu_mod_cfg), offsetof(dabgpu_mod_cfg, gain), offsetof(dabgpu_mod_cfg, tii_main), offsetof(dabgpu_mod_cfg, tii_sub));',
             '  printf("%d %d\\n", DABGPU_MOD_BAD_INPUT, DABGPU_MOD_MISALIGNED);', '  return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [[int(x) for x in l.split()] for l in subprocess.check_output([str(exe)], text=True).strip().split("\n")]
    dt = dabgpu.MOD_STATUS_DTYPE
    assert out[0] == [dt.itemsize, dt.fields["flags"][1], dt.fields["refused"][1]]
    assert out[1] == [C.sizeof(dabgpu.ModCfg), dabgpu.ModCfg.gain.offset, dabgpu.ModCfg.tii_main.offset, dabgpu.ModCfg.tii_sub.offset]
    assert out[2] == [dabgpu.MOD_BAD_INPUT, dabgpu.MOD_MISALIGNED] == [M.BAD_INPUT, M.MISALIGNED]


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def mctx(built):
    c = make_ctx(None, max_frames=64)
    yield c
    c.close()


def run_mod(ctx, eti, **kw):
    """eti: numpy [n_cif][6144] or [n_streams][n_cif][6144] -> (iq tensor [n_frames][stride], status records, state tensor)."""
    import torch
    e = np.asarray(eti)
    d = torch.from_numpy(np.array(e.reshape((-1,) + e.shape[-2:]) if e.ndim == 3 else e[None])).cuda()   # (a writable copy)
    iq, st, state = ctx.modulate_eti(d, streams(), **kw)
    return iq, st.cpu().numpy().view(dabgpu.MOD_STATUS_DTYPE).reshape(-1), state


@pytest.fixture(scope="module")
def device_iq(mctx, case):
    iq, st, _ = run_mod(mctx, case["eti"])
    return iq, st


def demod(ctx, iq):
    """device IQ tensor [n][stride] through dabgpu_ofdm_demod_frames_dev at zero offset -> soft tensor [n][230400]."""
    import torch
    n = iq.shape[0]
    soft = torch.zeros((n, synth.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
    fo = torch.zeros(n, dtype=torch.float32, device="cuda")
    ctx.ofdm_demod_frames_dev(iq.data_ptr() + 8 * synth.NB_NULL, iq.stride(0), n, fo.data_ptr(), soft.data_ptr())
    ctx.sync()
    return soft


@pytest.mark.gpu
def test_iq_against_the_reference(device_iq, case):
    """Every sample of the five frames; the worst value is printed.  DESIGN.md 4.4e records what was measured on the MI355X."""
    iq, st = device_iq
    got = iq.cpu().numpy()
    assert got.shape == (N_FRAMES, synth.NB_FRAME_SAMPLES)
    worst = worst_over_peak(got, case["iq"])
    print("modulator: worst |device - reference| / peak = %.3e (bound %.0e)" % (worst, IQ_BOUND))
    assert worst <= IQ_BOUND
    assert not st["flags"].any() and not st["refused"].any() and not st["reserved"].any()
    assert not got[:, :synth.NB_NULL].any()                     # default configuration: a null symbol of exact zeros


@pytest.mark.gpu
def test_bits_through_the_front_end(mctx, device_iq, case):
    soft = demod(mctx, device_iq[0]).cpu().numpy()
    hard = (soft > 0).astype(np.uint8)
    for f in range(N_FRAMES):
        wrong = np.nonzero(hard[f] != case["bits"][f])[0]
        if wrong.size:
            b = int(wrong[0])
            where = "FIC bit %d" % b if b < synth.NB_FIC_BITS else "CIF %d bit %d" % divmod(b - synth.NB_FIC_BITS, synth.NB_CIF_BITS)
            pytest.fail("frame %d: %d wrong bits, the first in data symbol %d (%s)" % (f, wrong.size, b // 3072 + 1, where))


@pytest.mark.gpu
def test_round_trip_to_eti_bytes(mctx, device_iq, case):
    """IQ -> front end -> channel decoder -> ETI writer: output frame t + 15 is input frame t, byte for byte."""
    import torch
    soft = demod(mctx, device_iq[0])
    sts = streams()
    plan = dabgpu.eti_layout(sts)
    scs = [sc for _, sc in sts]
    u8 = dict(dtype=torch.uint8, device="cuda")
    fib, ok = torch.zeros((N_FRAMES, 12, 32), **u8), torch.zeros((N_FRAMES, 12), **u8)
    outs = [torch.zeros((1, N_CIF, sc.bitrate_kbps * 3), **u8) for sc in scs]
    hist = [torch.zeros((1, 15, sc.length * 64), dtype=torch.int8, device="cuda") for sc in scs]
    eti, status = torch.zeros((1, N_CIF, 6144), **u8), torch.zeros((1, N_CIF, 8), **u8)
    start = torch.zeros(1, dtype=torch.int32, device="cuda")
    mctx.decode_frames_dev(soft.data_ptr(), soft.stride(0), 1, N_FRAMES, fib.data_ptr(), ok.data_ptr(), scs, None,
                           [h.data_ptr() for h in hist], [o.data_ptr() for o in outs])
    mctx.eti_frames_dev(plan, 1, N_FRAMES, fib.data_ptr(), ok.data_ptr(), [o.data_ptr() for o in outs], eti.data_ptr(),
                        status.data_ptr(), d_cif_start=start.data_ptr())
    mctx.sync()
    assert ok.cpu().numpy().all()
    got = eti.cpu().numpy()[0]
    for t in range(N_CIF - 15):
        assert got[t + 15].tobytes() == case["eti"][t].tobytes(), t
        dabgpu.eti_parse(got[t + 15])


@pytest.mark.gpu
def test_chained_calls_equal_one(mctx, device_iq, case):
    import torch
    one = device_iq[0]
    a, _, state = run_mod(mctx, case["eti"][:8])
    b, _, state2 = run_mod(mctx, case["eti"][8:], state=state)
    assert torch.equal(torch.cat([a, b]), one)
    # a call shorter than the interleaver's depth carries the older CIFs on: 1 + 1 + 3 frames
    c1, _, s1 = run_mod(mctx, case["eti"][:4])
    c2, _, s2 = run_mod(mctx, case["eti"][4:8], state=s1)
    c3, _, s3 = run_mod(mctx, case["eti"][8:], state=s2)
    assert torch.equal(torch.cat([c1, c2, c3]), one) and torch.equal(s2, state) and torch.equal(s3, state2)
    # no state and an all-zero state are the same start
    z, _, sz = run_mod(mctx, case["eti"], state=torch.zeros((1, dabgpu.mod_state_bytes()), dtype=torch.uint8, device="cuda"))
    assert torch.equal(z, one) and torch.equal(sz, state2)


@pytest.mark.gpu
def test_batch_and_stride(mctx, device_iq, case):
    import torch
    etis = [case["eti"]] + [M.build_eti(REF, *contents(seed)) for seed in (101, 102)]
    alone = [device_iq[0]] + [run_mod(mctx, e)[0] for e in etis[1:]]
    assert not torch.equal(alone[1], alone[2])
    stride = synth.NB_FRAME_SAMPLES + 64
    out = torch.full((3 * N_FRAMES, stride), 7.0 + 3.0j, dtype=torch.complex64, device="cuda")
    iq, st, _ = run_mod(mctx, np.stack(etis), frame_stride=stride, out=out)
    assert iq.data_ptr() == out.data_ptr() and not st["flags"].any()
    for s in range(3):
        assert torch.equal(iq[s * N_FRAMES:(s + 1) * N_FRAMES, :synth.NB_FRAME_SAMPLES], alone[s]), s
    assert bool((iq[:, synth.NB_FRAME_SAMPLES:] == 7.0 + 3.0j).all())


@pytest.mark.gpu
def test_tii_null_symbol(mctx, device_iq, case):
    import torch
    c, p = 11, 37
    iq, _, _ = run_mod(mctx, case["eti"], cfg=dabgpu.mod_cfg(tii_main=p, tii_sub=c))
    assert torch.equal(iq[:, synth.NB_NULL:], device_iq[0][:, synth.NB_NULL:])
    got = iq.cpu().numpy()
    want = synth.tii_null([(c, p)])
    peak = np.abs(case["iq"]).max(axis=1)
    worst = max(float(np.abs(got[f, :synth.NB_NULL].astype(np.complex128) - want).max() / peak[f]) for f in range(N_FRAMES))
    print("modulator: TII null symbol, worst |device - reference| / peak = %.3e" % worst)
    assert worst <= IQ_BOUND
    # the detector's threshold is relative to the noise floor it measures beside the ensemble: on a noise-free signal that
    # floor is the transform's rounding (1e-14 of a carrier) and cells of rounding residue pass it, so the signal gets
    # white noise 20 dB below its unit power, as a receiver would see it
    rng = np.random.default_rng(5)
    noise = np.sqrt(0.005) * (rng.standard_normal(got.shape) + 1j * rng.standard_normal(got.shape))
    rx = torch.from_numpy((got + noise).astype(np.complex64)).cuda()
    acc = torch.zeros(dabgpu.TII_ACC_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    fo = torch.zeros(N_FRAMES, dtype=torch.float32, device="cuda")
    mctx.tii_frames_dev(rx.data_ptr() + 8 * synth.NB_NULL, rx.stride(0), 1, N_FRAMES, acc.data_ptr(), d_freq_offset=fo.data_ptr())
    mctx.sync()
    found = dabgpu.tii_decode(acc.cpu().numpy().view(dabgpu.TII_ACC_DTYPE)[0])
    assert [(int(e["main_id"]), int(e["sub_id"])) for e in found] == [(p, c)]
    # another transmitter, then none again: the table follows the configuration
    other, _, _ = run_mod(mctx, case["eti"][:4], cfg=dabgpu.mod_cfg(tii_main=0, tii_sub=23))
    assert np.abs(other.cpu().numpy()[0, :synth.NB_NULL] - synth.tii_null([(23, 0)])).max() <= IQ_BOUND * peak[0]
    again, _, _ = run_mod(mctx, case["eti"])
    assert torch.equal(again, device_iq[0])


@pytest.mark.gpu
def test_refused_input_frames(mctx, device_iq, case):
    import torch
    eti = case["eti"].copy()
    eti[6, 2] ^= 0x08                                           # FSYNC
    eti[13, 9] ^= 0x01                                          # the start address in the first STC word
    iq, st, _ = run_mod(mctx, eti)
    assert [(int(x["flags"]), int(x["refused"])) for x in st] == M.status(eti, refused=(6, 13)) == \
        [(0, 0), (1, 4), (0, 0), (1, 2), (0, 0)]
    want = M.modulate(M.frame_bits(REF, case["fibs"], case["data"], refused=(6, 13)))
    worst = worst_over_peak(iq.cpu().numpy(), want)
    print("modulator: refused input, worst |device - reference| / peak = %.3e" % worst)
    assert worst <= IQ_BOUND
    soft = demod(mctx, iq).cpu().numpy()
    assert ((soft > 0).astype(np.uint8) == M.frame_bits(REF, case["fibs"], case["data"], refused=(6, 13))).all()
    # the frame before the first refused one is untouched; the interleaver spreads the zero bytes over the later ones
    assert torch.equal(iq[0], device_iq[0][0]) and not torch.equal(iq[2], device_iq[0][2])


@pytest.mark.gpu
def test_gain_and_misalignment(mctx, device_iq, case):
    import torch
    half, _, _ = run_mod(mctx, case["eti"], cfg=dabgpu.mod_cfg(gain=0.5))
    assert torch.equal(half, device_iq[0] * 0.5)
    tii, _, _ = run_mod(mctx, case["eti"][:4], cfg=dabgpu.mod_cfg(gain=0.5, tii_main=5, tii_sub=6))
    full, _, _ = run_mod(mctx, case["eti"][:4], cfg=dabgpu.mod_cfg(tii_main=5, tii_sub=6))
    assert torch.equal(tii, full * 0.5)
    # the same contents counted from CIF 2: every transmission frame begins with FP mod 4 = 2, flagged and modulated all the same
    shifted = M.build_eti(REF, case["fibs"], case["data"], count0=2)
    iq, st, _ = run_mod(mctx, shifted)
    assert [(int(x["flags"]), int(x["refused"])) for x in st] == M.status(shifted) == [(dabgpu.MOD_MISALIGNED, 0)] * N_FRAMES
    assert torch.equal(iq, device_iq[0])


@pytest.mark.gpu
def test_refused_calls_enqueue_nothing(mctx, case):
    import torch
    sts = streams()
    plan = dabgpu.eti_layout(sts)
    eti = torch.from_numpy(case["eti"].copy()).cuda()
    iq = torch.zeros((N_FRAMES, synth.NB_FRAME_SAMPLES), dtype=torch.complex64, device="cuda")
    st = torch.full((N_FRAMES, 8), 0xEE, dtype=torch.uint8, device="cuda")
    state = torch.zeros((1, dabgpu.mod_state_bytes()), dtype=torch.uint8, device="cuda")
    args = lambda **kw: dict(dict(plan=plan, streams=sts, n_streams=1, frames_per_stream=N_FRAMES, d_eti=eti.data_ptr(),
                                  d_iq=iq.data_ptr(), d_status=st.data_ptr()), **kw)
    wrong = [(i, dabgpu.Subchannel(sc.start_address, sc.length + 1, sc.is_uep, sc.eep_type, sc.protection_level, sc.bitrate_kbps))
             for i, sc in sts]
    for kw, code in ((dict(d_iq=iq.data_ptr() + 8), -1), (dict(frame_stride=196609), -1), (dict(streams=wrong), -5),
                     (dict(d_state_in=state.data_ptr(), d_state_out=state.data_ptr()), -1),
                     (dict(cfg=dabgpu.mod_cfg(tii_main=70, tii_sub=1)), -1), (dict(d_status=st.data_ptr() + 4), -1)):
        with pytest.raises(dabgpu.DabGpuError) as e:
            mctx.modulate_eti_dev(**args(**kw))
        assert e.value.status == code, kw
    mctx.sync()
    assert not iq.any() and bool((st == 0xEE).all())
    mctx.set_timing(True)
    mctx.modulate_eti_dev(**args())
    assert mctx.last_kernel_ms(dabgpu.WHICH_MOD_ENCODE) > 0 and mctx.last_kernel_ms(dabgpu.WHICH_MOD_SYMBOLS) > 0
    assert mctx.mean_kernel_ms(dabgpu.WHICH_MOD_ENCODE)[1] == 1 and mctx.mean_kernel_ms(dabgpu.WHICH_MOD_SYMBOLS)[1] == 1
    mctx.set_timing(False)
    assert iq.any() and not st.any()
