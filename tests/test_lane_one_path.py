"""The seams of the lane decoder's one launch path.  Single items -- plain codewords, the FIC alone, one sub-channel --
have no traceback of their own any more: where they can take a fused forward pass (a sub-channel as a pack of one entry of
the grouped kernel, the FIC and plain codewords on the 64-row forward kernel) and where they cannot (prep kernel -> forward
pass on soft words), the traceback is the grouped one on a pack of one.  Only a list that went out as ONE forward and ONE
traceback launch has timer parts.  Every case: the lane kernels forced (FLAG_VITERBI_LANE) against the wave-per-codeword
kernels (FLAG_VITERBI_WAVE) and against tests/decoder_reference.py, bit for bit (the reference under the tie rule the
kernels document)."""
import functools

import numpy as np
import pytest

import decoder_reference as R
from conftest import make_ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lane(built):
    c = make_ctx(1, max_frames=8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wave(built):
    c = make_ctx(0, max_frames=8)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ plain codewords
PLAIN_STEPS = 198                                            # 792 mother bits


@functools.lru_cache(maxsize=None)
def plain_case(punctured):
    """-> mask, punctured soft bits int8 [130][kept], the reference's bytes [130][24].  punctured: 784 of the 792 mother
    bits are kept (a multiple of 16: every codeword starts on a 16-byte boundary, the fused forward pass); else all 792
    (not a multiple of 16: the prep kernel, on a source that has no interleaving)."""
    mask = np.ones(4 * PLAIN_STEPS, np.uint8)
    if punctured:
        mask[3:792:100] = 0
    kept = int(mask.sum())
    assert kept == (784 if punctured else 792) and (kept % 16 == 0) == punctured
    rng = np.random.default_rng(198 + punctured)
    punct = rng.integers(-127, 128, (130, kept)).astype(np.int8)
    return mask, punct, R.viterbi(R.depuncture(punct, mask), stats=False).bytes()


@pytest.mark.parametrize("punctured", [True, False])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 130])
def test_plain_codewords_as_a_pack_of_one(lane, wave, n, punctured):
    """Codeword counts that are no multiple of 4 (the frame-shaped source splits codeword g into row g >> 2, part g & 3)
    and the ends of a 64-codeword group (lanes past the end repeat the last codeword)."""
    mask, punct, want = plain_case(punctured)
    got = lane.viterbi(punct[:n], mask)
    assert (got == wave.viterbi(punct[:n], mask)).all()
    assert (got == want[:n]).all()


# ------------------------------------------------------------------------------------------------ the FIC alone
@functools.lru_cache(maxsize=None)
def fic_case():
    """-> FIC soft bits int8 [17][9216] and the reference.  Even frames carry FIBs with a good CRC under noise, odd frames are
    noise alone, so both values of the CRC flag occur."""
    rng = np.random.default_rng(774)
    p = R.fic_profile()
    soft = rng.integers(-127, 128, (17, 9216)).astype(np.int8)
    for f in range(0, 17, 2):
        fibs = np.stack([R.fib_with_crc(rng.integers(0, 256, 30)) for _ in range(12)])
        bits = np.unpackbits(fibs.reshape(4, 96), axis=1) ^ R.prbs(768)[None, :]
        code = R.conv_encode(bits)[:, np.flatnonzero(p.mask)].astype(np.float64) * 2 - 1
        soft[f] = np.clip(np.rint(50 * code + rng.normal(0, 40, code.shape)), -127, 127).astype(np.int8).reshape(-1)
    ref = R.fic_reference(soft)
    assert ref.crc_ok[0::2].all() and not ref.crc_ok[1::2].all()
    return soft, ref


@pytest.mark.parametrize("layout", ["stride 230400", "stride 9216", "offset 1"])
@pytest.mark.parametrize("n_frames", [1, 15, 16, 17])
def test_fic_alone_as_a_pack_of_one(lane, wave, n_frames, layout):
    """4, 60, 64 and 68 codewords through dabgpu_fic_decode_dev: aligned frames (whole frames and FIC-only ones) take the
    fused forward pass, frames that start on an odd byte the prep kernel with the forced delay."""
    import torch
    soft, ref = fic_case()
    dev = torch.device("cuda", 0)
    stride = 9216 if layout == "stride 9216" else 230400
    off = 1 if layout == "offset 1" else 0
    buf = torch.zeros(n_frames * stride + 16, dtype=torch.int8, device=dev)
    buf[off:off + n_frames * stride].view(n_frames, stride)[:, :9216] = torch.from_numpy(soft[:n_frames]).to(dev)
    assert buf.data_ptr() % 16 == 0
    res = []
    for c in (lane, wave):
        fib = torch.zeros((n_frames, 12, 32), dtype=torch.uint8, device=dev)
        ok = torch.full((n_frames, 12), 7, dtype=torch.uint8, device=dev)
        c.fic_decode_dev(buf.data_ptr() + off, stride, n_frames, fib.data_ptr(), ok.data_ptr(), None)
        c.sync()
        res.append((fib.cpu().numpy(), ok.cpu().numpy()))
    assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()
    assert (res[0][0] == ref.fib[:n_frames]).all() and (res[0][1] == ref.crc_ok[:n_frames]).all()


# ------------------------------------------------------------------------------------------------ one sub-channel
MSC_STREAMS, MSC_START_CU = 3, 21


@functools.lru_cache(maxsize=None)
def msc_case(fps):
    """-> frames int8 [3 fps][230400] (noise everywhere), history rings int8 [3][15][nbits], the reference per stream."""
    p = R.eep_profile(0, 3, 32)                              # 32 kbit/s EEP 3-A: 774 steps, 24 capacity units
    nbits = p.size_cu * 64
    rng = np.random.default_rng(1000 + fps)
    frames = rng.integers(-127, 128, (MSC_STREAMS * fps, 230400)).astype(np.int8)
    hist = rng.integers(-127, 128, (MSC_STREAMS, 15, nbits)).astype(np.int8)
    cifs = frames[:, 9216:].reshape(MSC_STREAMS, fps * 4, 55296)[:, :, MSC_START_CU * 64:MSC_START_CU * 64 + nbits]
    return frames, hist, [R.msc_reference(cifs[s], hist[s], p) for s in range(MSC_STREAMS)]


@pytest.mark.parametrize("fps", [16, 6])
def test_one_sub_channel_with_history_in_and_out(lane, wave, fps):
    """3 streams through dabgpu_msc_decode_dev with carried history: 16 frames per stream are whole 64-codeword groups (a
    fused pack of one), 6 frames per stream are not (groups straddle streams: the prep kernel).  Every codeword and the
    rings the call leaves behind."""
    import dabgpu
    frames, hist, refs = msc_case(fps)
    sc = dabgpu.subchannel(MSC_START_CU, 32, level=3)
    got = lane.msc_decode(sc, frames, MSC_STREAMS, history_in=hist, want_history=True)
    other = wave.msc_decode(sc, frames, MSC_STREAMS, history_in=hist, want_history=True)
    assert (got[0] == other[0]).all() and (got[1] == other[1]).all()
    for s, r in enumerate(refs):
        assert (got[0][s] == r.out).all(), s
        assert (got[1][s] == r.history).all(), s


# ------------------------------------------------------------------------------------------------ the timer's parts
def test_a_list_cut_into_several_packs_has_no_timer_parts():
    """30 sub-channels, 16 frames, the lane kernels forced: two packs (16 + 14 entries), so two forward and two traceback
    launches -- no single pair of events splits that call.  The whole call's slot answers; the parts say that there is no
    such number (DABGPU_ERR_ARG), never the figure of one pack."""
    import dabgpu
    import torch
    dev = torch.device("cuda", 0)
    fps = 16
    scs = [dabgpu.subchannel(6 * i, 8, level=3) for i in range(30)]
    g = torch.Generator(device=dev); g.manual_seed(4242)
    soft = torch.randint(-127, 128, (fps, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev, generator=g)
    outs = [torch.zeros((1, fps * 4, sc.bitrate_kbps * 3), dtype=torch.uint8, device=dev) for sc in scs]
    hout = [torch.zeros((1, 15, sc.length * 64), dtype=torch.int8, device=dev) for sc in scs]
    c = make_ctx(1, max_frames=8)
    try:
        c.set_timing(True)
        c.msc_decode_multi_dev(scs, soft.data_ptr(), dabgpu.NB_FRAME_BITS, 1, fps, None, [h.data_ptr() for h in hout],
                               [o.data_ptr() for o in outs], None)
        c.sync()
        whole, calls = c.mean_kernel_ms(2)
        assert calls == 1 and whole > 0
        for which in (4, 5, 6):
            with pytest.raises(dabgpu.DabGpuError):
                c.mean_kernel_ms(which)
        c.set_timing(False)
    finally:
        c.close()
