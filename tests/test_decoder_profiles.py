"""Every protection profile on every decoder path, bit for bit (rows A12 and f-2 of tests/README.md, and the BER part of
the measurement row): all 64 UEP rows, EEP-A 1..4 at 8 / 16 / 24 / 72 kbit/s and EEP-B 1..4 at 32 / 96 kbit/s, 88 profiles
of 18 codeword lengths packed into 9 streams (tests/decoder_profiles.py), against tests/decoder_reference.py through the
assertion test_decoder_reference.py uses: maximum likelihood by metric first, the documented tie rule's bytes second.

Each device path reads a table of its own that is derived per profile -- the wave kernels d_mother_pos and its chunk
table, the lane kernels d_punct_idx, the fused forward pass its 24-step tiles, the BER kernel d_punct_idx again -- and a
wrong entry loses or misplaces a few soft bits, which the code corrects on any input that carries a signal.  So most of
each profile's 16 codewords are noise (uniform, and a 16-level grid with many exact ties), whose optimum moves with a
single soft bit, and the CPU part MEASURES that: every structural mutant of the reference (a block boundary, one block's
PI, the tail's vector, the start bit, the padding) must be rejected for every profile, and of the single-bit mutants
(one kept soft bit erased or exchanged with its neighbour, profiles up to 1 158 steps) at most 10 % may pass per profile.

`-m gpu`, each launch form on the shape that reaches it, and the form asserted where the library lets a test see it:
  - four frames (16 codewords): msc_decode on the wave kernels and on the lane kernels behind the prep kernel (an item
    that is no whole 64-codeword group goes through the prep kernel); decode_frames on the wave kernels, the small-batch
    grouped wave launch (one timed slot);
  - sixteen frames (the period four times, one 64-codeword group per entry): msc_decode_dev on the lane kernels, a fused
    pack of one; decode_frames_dev on the lane kernels, entries by value in packs of 16 (one timed slot; timer parts for
    one pack, none for the 31-entry stream's two); decode_ensembles_dev over all 9 streams, entries by table (one slot
    with parts), and the same call at four frames a stream, part by part;
  - the channel BER of random "decoded" bytes, where every kept bit counts whatever the code's strength."""
import functools

import numpy as np
import pytest

import decoder_profiles as P
import decoder_reference as R
import quality_reference as QR
from conftest import make_ctx

MISS_CAP = 0.10                                          # single-bit mutants that may pass, per profile
FB = P.NB_FRAME_BITS


def _report(line):
    print("\n[decoder_profiles] " + line)


def _rejected(got, mother, d, what):
    try:
        R.assert_decoder(got, mother, d, True, what)
    except AssertionError:
        return True
    return False


# ================================================================================================ CPU
def test_coverage_is_what_the_module_claims():
    keys = P.PROFILES
    assert len(keys) == len(set(keys)) == 88
    assert sorted(k[1] for k in keys if k[0] == "uep") == list(range(64))
    assert sorted(k[2:] for k in keys if k[:2] == ("eep", 0)) == sorted((lv, br) for lv in (1, 2, 3, 4) for br in (8, 16, 24, 72))
    assert sorted(k[2:] for k in keys if k[:2] == ("eep", 1)) == sorted((lv, br) for lv in (1, 2, 3, 4) for br in (32, 96))
    assert P.profile(("eep", 0, 2, 8)).blocks == [(5, 13), (1, 12)]               # the special case at 8 kbit/s
    every = set()
    for opt, rates in ((0, range(8, 1729, 8)), (1, range(32, 1729, 32))):
        for lv in (1, 2, 3, 4):
            every |= {pi for br in rates for n, pi in R.eep_profile(opt, lv, br).blocks if n > 0}
    every |= {pi for i in range(64) for n, pi in R.uep_profile(i).blocks if n > 0}
    used = {pi for k in keys for pi in P.block_pis(P.profile(k))}
    assert every == set(range(1, 25)) - {21}                                       # (PI 21 is in no profile of the standard)
    assert used == every, sorted(every - used)                                     # every index that occurs in any profile
    assert len(P.LENGTHS) == 18 and (P.LENGTHS[0], P.LENGTHS[-1]) == (198, 9222)
    assert sum(P.profile(k).size_cu for k in keys) == 7709
    assert sum(1 for k in keys if P.profile(k).padding) == 21
    st = P.streams()
    assert len(st) == 9 and sorted(k for lst in st for k, _ in lst) == sorted(keys)
    assert (min(len(lst) for lst in st), max(len(lst) for lst in st)) == (3, 31)   # one list longer than a pack of 16
    gaps = 0
    for lst in st:
        at = 0
        for j, (k, start) in enumerate(lst):
            p = P.profile(k)
            assert start >= at and start + p.size_cu <= 864
            gaps += start > at
            if p.padding:                                                          # followed directly by another entry
                assert j + 1 < len(lst) and lst[j + 1][1] == start + p.size_cu, P.name(k)
            at = start + p.size_cu
    assert all(lst[0][1] == 0 for lst in st) and gaps >= 2
    assert sum(lst[-1][1] + P.profile(lst[-1][0]).size_cu == 864 for lst in st) >= 2


def test_builder_takes_nothing_from_the_code_under_test():
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "decoder_profiles.py")).read()
    imports = sorted(l.strip() for l in src.splitlines() if l.strip().startswith(("import ", "from ")))
    assert imports == ["import decoder_reference as R", "import functools", "import numpy as np"], imports


@pytest.mark.parametrize("s", range(9))
def test_streams_deinterleave_to_the_codewords(s):
    """The reference's time_deinterleave over the built stream gives back the 16 codewords exactly, history_out is the
    last 15 rows and equals history_in (the transmission is cyclic), a longer run repeats them, and the clean codewords
    come back as their messages."""
    frames = P.stream_frames(s)
    cifs = frames[:, R.NB_FIC_BITS:].reshape(16, R.NB_CIF_BITS)
    for k, start in P.streams()[s]:
        p = P.profile(k)
        c, msgs = P.codewords(k)
        sub = cifs[:, 64 * start:64 * (start + p.size_cu)]
        assert (sub == P.period(k)).all()
        lf, hist = R.time_deinterleave(sub, P.history(k))
        assert (lf[:, :p.kept] == c).all(), P.name(k)
        assert (hist == sub[-15:]).all() and (hist == P.history(k)).all()
        lf2, _ = R.time_deinterleave(np.tile(sub, (2, 1)), P.history(k))
        assert (lf2[:, :p.kept] == np.tile(c, (2, 1))).all()
        assert np.abs(c[list(P.CLEAN)].astype(int)).min() == 127 and len(np.unique(c[10:])) <= 16
        _, d = P.ref(k)
        assert (d.bits()[list(P.CLEAN)] == msgs).all() and msgs[1].all(), P.name(k)
        if p.padding:
            assert np.abs(sub[:, p.kept:].astype(int)).max() > 100                 # noise, not erasures


@pytest.mark.parametrize("nsteps", P.LENGTHS)
def test_oracle_on_every_profile(built, nsteps):
    from oracle import oracle as O
    for k in P.keys_of_length(nsteps):
        p = P.profile(k)
        mother, d = P.ref(k)
        rows = np.concatenate([P.history(k), P.period(k)])
        got = np.stack([O.msc_decode_lf(O.time_deinterleave(rows[t:t + 16])[:p.kept], p.mask, p.nsteps) for t in range(16)])
        R.assert_decoder(got, mother, d, True, "oracle, " + P.name(k))


@pytest.mark.parametrize("nsteps", P.LENGTHS)
def test_structural_mutants_are_rejected(nsteps):
    """A hard condition on the sweep, by the reference alone: a decoder whose table is wrong in one structural respect
    -- the first puncturing region one 32-step block longer, one block's PI changed by one, the tail's vector shifted by
    one, the sub-channel read one bit late, (UEP with padding) the tail bits taken from the padding -- returns bytes the
    assertion rejects, for every profile and every mutant.  Judged on the 12 noise codewords of the same soft bits: what
    they reject, the 16 reject."""
    cases = [(k, kind, P.mutant_mother(k, kind)) for k in P.keys_of_length(nsteps) for kind in P.STRUCTURAL]
    cases = [c for c in cases if c[2] is not None]
    assert len(cases) == sum(4 + bool(P.profile(k).padding) for k in P.keys_of_length(nsteps))
    got = P.reference_bytes(np.concatenate([m for _, _, m in cases]))
    passed = []
    for i, (k, kind, _) in enumerate(cases):
        mother, d = P.noise_ref(k)
        if not _rejected(got[12 * i:12 * (i + 1)], mother, d, kind):
            passed.append((P.name(k), kind))
    assert not passed, passed


@pytest.mark.parametrize("nsteps", P.SHORT_LENGTHS)
def test_single_bit_mutants_are_rejected(nsteps):
    """One kept soft bit erased, or exchanged with its neighbour, in every codeword at once (what a wrong table entry
    does): at most 10 % of these mutants may pass the assertion, per profile.  Positions: the first and last kept bit of
    every puncturing region and of the tail, both sides of every eighth 24-step tile boundary, 4 seeded random ones (the
    sample is cut for run time, as is the range: the profiles above 1 158 steps are left out).  Judged on the 12 noise
    codewords, which can only overstate the share.  Measured: 5.0 / 0 / 3.6 / 3.1 / 2.1 % for the worst profile of 198 /
    390 / 582 / 774 / 1 158 steps (EEP 1-A at 8 and 24 kbit/s lead: the strongest code on the shortest codewords)."""
    assert nsteps <= 1158
    worst = (-1.0, "")
    for k in P.keys_of_length(nsteps):
        labels, mutants = P.single_bit_mutants(k)
        got = P.reference_bytes(mutants.reshape(-1, mutants.shape[2])).reshape(len(labels), len(P.NOISE), -1)
        mother, d = P.noise_ref(k)
        passed = [lab for lab, g in zip(labels, got) if not _rejected(g, mother, d, lab)]
        share = len(passed) / len(labels)
        _report("single-bit mutants, %-9s (%4d steps): %2d of %3d pass (%.1f %%)" % (P.name(k), nsteps, len(passed), len(labels), 100 * share))
        worst = max(worst, (share, P.name(k)))
        assert share <= MISS_CAP, (P.name(k), passed)
    _report("single-bit mutants, %d steps: worst share %.1f %% (%s)" % (nsteps, 100 * worst[0], worst[1]))


# ================================================================================================ GPU
def _sc(key):
    import dabgpu
    _, _, start = P.place(key)
    p = P.profile(key)
    sc = dabgpu.uep_subchannel(key[1], start) if key[0] == "uep" else dabgpu.subchannel(start, key[3], level=key[2], eep_type=key[1])
    assert sc.length == p.size_cu and sc.bitrate_kbps * 3 == p.nbytes and sc.start_address == start
    return sc


def _to_dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))      # (a copy: the builder's arrays are read-only)


def _msc_slots(c):
    """With timing on since set_timing(True): how many timed msc / grouped slots the calls since left, and how many of
    them have the parts (forward | traceback | history) that only ONE forward and ONE traceback launch leaves."""
    import dabgpu
    _, slots = c.mean_kernel_ms(2)
    try:
        _, parts = c.mean_kernel_ms(4)
    except dabgpu.DabGpuError:
        parts = 0
    return slots, parts


@pytest.fixture(scope="module", params=["wave", "prep lane"])
def path_ctx(built, request):
    c = make_ctx(0) if request.param == "wave" else make_ctx(1, unfused=True)
    yield request.param, c
    c.close()


@pytest.fixture(scope="module")
def wave_ctx(built):
    c = make_ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lane_ctx(built):
    c = make_ctx(1)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nsteps", P.LENGTHS)
def test_gpu_msc_decode_of_every_profile(path_ctx, nsteps):
    """dabgpu_msc_decode, n_streams = 1: each profile on its stream's four frames with the carried history, on the wave
    kernels (d_mother_pos and its chunk table) and on the lane kernels behind lane_prep_kernel (d_punct_idx).  Four frames
    are 16 codewords, no whole 64-codeword group: the lane kernels take such an item through the prep kernel whether
    the context says unfused or not, so this is no test of the fused forward pass."""
    path, c = path_ctx
    for k in P.keys_of_length(nsteps):
        s, _, _ = P.place(k)
        mother, d = P.ref(k)
        out, ho = c.msc_decode(_sc(k), P.stream_frames(s), 1, history_in=P.history(k)[None], want_history=True)
        R.assert_decoder(out[0], mother, d, True, "%s, msc_decode, %s" % (path, P.name(k)))
        assert (ho[0] == P.history(k)).all(), (path, P.name(k))


def _assert_fic(fib, ok, ref, what):
    R.assert_decoder(fib.reshape(-1, 96), ref.mother, ref.decoded, True, what + ", FIC")
    assert (ok.reshape(-1, 12) == ref.crc_ok).all(), what


def _assert_four_periods(out, key, what):
    """out [64][nbytes] of 16 frames = the four-frame period four times: the repetitions identical, the first 16 codewords
    through the assertion."""
    mother, d = P.ref(key)
    got = out.reshape(4, 16, -1)
    assert (got == got[0]).all(), "%s: the four copies of a codeword differ, %s" % (what, P.name(key))
    R.assert_decoder(got[0], mother, d, True, "%s, %s" % (what, P.name(key)))


@functools.lru_cache(maxsize=None)
def _sixteen_frames(s):
    return _to_dev(np.tile(P.stream_frames(s), (4, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("nsteps", P.LENGTHS)
def test_gpu_fused_msc_decode_of_every_profile(lane_ctx, nsteps):
    """The fused forward pass (fused_desc / fused_tiles) on a single item: dabgpu_msc_decode_dev with the lane kernels
    forced, one stream of 16 frames = exactly one 64-codeword group.  A single item leaves no timer parts, so which
    forward pass ran cannot be read back; what the test does is meet every condition of lane_item_fusable
    (csrc/lane_plan.hpp) and assert the ones it controls -- whole groups, 16-byte aligned soft bits, stride, history
    and output -- so that the item goes out as one fused pack of one (the start bit, 9216 + 64 start CU, and the row
    length 64 size CU are multiples of 16 for every sub-channel; the context is not unfused)."""
    import torch
    dev = torch.device("cuda", 0)
    for k in P.keys_of_length(nsteps):
        p = P.profile(k)
        soft = _sixteen_frames(P.place(k)[0])
        hin = _to_dev(P.history(k))
        hout = torch.zeros((15, 64 * p.size_cu), dtype=torch.int8, device=dev)
        out = torch.zeros((64, p.nbytes), dtype=torch.uint8, device=dev)
        assert soft.shape[0] * 4 % 64 == 0 and FB % 16 == 0
        assert all(x.data_ptr() % 16 == 0 for x in (soft, hin, hout, out))
        lane_ctx.msc_decode_dev(_sc(k), soft.data_ptr(), FB, 1, 16, hin.data_ptr(), hout.data_ptr(), out.data_ptr(), None)
        lane_ctx.sync()
        _assert_four_periods(out.cpu().numpy(), k, "fused lane, msc_decode_dev")
        assert (hout.cpu().numpy() == P.history(k)).all(), P.name(k)


@pytest.mark.gpu
@pytest.mark.parametrize("s", range(9))
def test_gpu_wave_decode_frames_of_every_stream(wave_ctx, s):
    """dabgpu_decode_frames on the wave kernels: a stream's whole list (3 .. 31 entries) on four frames with the FIC,
    the small-batch grouped wave launch -- asserted: the call leaves ONE timed slot, where the FIC alone and one call
    per sub-channel would leave as many as the list has entries."""
    keys = [k for k, _ in P.streams()[s]]
    wave_ctx.set_timing(True)
    try:
        fib, ok, outs, hos = wave_ctx.decode_frames(P.stream_frames(s), 1, [_sc(k) for k in keys],
                                                    history_in=[P.history(k)[None] for k in keys], want_history=True)
        assert _msc_slots(wave_ctx) == (1, 0)
    finally:
        wave_ctx.set_timing(False)
    for k, out, ho in zip(keys, outs, hos):
        mother, d = P.ref(k)
        R.assert_decoder(out[0], mother, d, True, "wave, decode_frames, stream %d, %s" % (s, P.name(k)))
        assert (ho[0] == P.history(k)).all(), P.name(k)
    _assert_fic(fib, ok, P.fic_ref(s), "wave, decode_frames, stream %d" % s)


@pytest.mark.gpu
@pytest.mark.parametrize("s", range(9))
def test_gpu_fused_decode_frames_of_every_stream(lane_ctx, s):
    """dabgpu_decode_frames_dev with the lane kernels forced, 16 frames: the FIC and the stream's list as entries BY VALUE
    of the grouped fused launch, at most 16 a pack.  Asserted: the call leaves ONE timed slot (sent one by one it would
    leave one per sub-channel), and a list of up to 15 entries -- one pack with the FIC -- leaves the timer parts of one
    forward and one traceback launch, while the 31-entry stream, two packs, leaves none."""
    import torch
    dev = torch.device("cuda", 0)
    keys = [k for k, _ in P.streams()[s]]
    soft = _sixteen_frames(s)
    hin = [_to_dev(P.history(k)) for k in keys]
    hout = [torch.zeros((15, 64 * P.profile(k).size_cu), dtype=torch.int8, device=dev) for k in keys]
    outs = [torch.zeros((64, P.profile(k).nbytes), dtype=torch.uint8, device=dev) for k in keys]
    fib = torch.zeros((16, 12, 32), dtype=torch.uint8, device=dev)
    ok = torch.zeros((16, 12), dtype=torch.uint8, device=dev)
    assert all(x.data_ptr() % 16 == 0 for x in [soft, fib] + hin + hout + outs)
    lane_ctx.set_timing(True)
    try:
        lane_ctx.decode_frames_dev(soft.data_ptr(), FB, 1, 16, fib.data_ptr(), ok.data_ptr(), [_sc(k) for k in keys],
                                   [h.data_ptr() for h in hin], [h.data_ptr() for h in hout], [o.data_ptr() for o in outs], None)
        lane_ctx.sync()
        assert _msc_slots(lane_ctx) == (1, 1 if len(keys) + 1 <= 16 else 0), len(keys)
    finally:
        lane_ctx.set_timing(False)
    assert max(len(lst) for lst in P.streams()) + 1 > 16                            # (stream 8 is the case of two packs)
    for k, out, ho in zip(keys, outs, hout):
        _assert_four_periods(out.cpu().numpy(), k, "fused lane, decode_frames_dev, stream %d" % s)
        assert (ho.cpu().numpy() == P.history(k)).all(), P.name(k)
    ref = P.fic_ref(s)
    f, o = fib.cpu().numpy().reshape(4, 4, 12, 32), ok.cpu().numpy().reshape(4, 4, 12)
    assert (f == f[0]).all() and (o == o[0]).all()
    _assert_fic(f[0], o[0], ref, "fused lane, decode_frames_dev, stream %d" % s)


def _ragged(c, fps):
    """One dabgpu_decode_ensembles_dev over the 9 streams, fps frames each (the four-frame period repeated), every entry
    with its history_in, the FIC in the same launch.  -> fib, ok, {key: out [4 fps][nbytes]}, {key: history_out}"""
    import torch
    dev = torch.device("cuda", 0)
    st = P.streams()
    soft = _to_dev(np.concatenate([np.tile(P.stream_frames(s), (fps // 4, 1)) for s in range(9)]))
    scs = [[_sc(k) for k, _ in lst] for lst in st]
    hin = [[_to_dev(P.history(k)) for k, _ in lst] for lst in st]
    hout = [[torch.zeros((15, 64 * P.profile(k).size_cu), dtype=torch.int8, device=dev) for k, _ in lst] for lst in st]
    outs = [[torch.zeros((4 * fps, P.profile(k).nbytes), dtype=torch.uint8, device=dev) for k, _ in lst] for lst in st]
    fib = torch.zeros((9 * fps, 12, 32), dtype=torch.uint8, device=dev)
    ok = torch.zeros((9 * fps, 12), dtype=torch.uint8, device=dev)
    ptr = lambda lsts: [[t.data_ptr() for t in lst] for lst in lsts]
    c.decode_ensembles_dev(soft.data_ptr(), FB, 9, fps, fib.data_ptr(), ok.data_ptr(), scs, ptr(hin), ptr(hout), ptr(outs), None)
    c.sync()
    flat = [k for lst in st for k, _ in lst]
    return (fib.cpu().numpy(), ok.cpu().numpy(), dict(zip(flat, [o.cpu().numpy() for lst in outs for o in lst])),
            dict(zip(flat, [h.cpu().numpy() for lst in hout for h in lst])))


@pytest.mark.gpu
def test_gpu_ragged_by_table_launch(built):
    """All 9 streams x 16 frames in one call (exactly one 64-codeword group per entry: the grouped launch, entries given
    by table), then the same call at 4 frames a stream, which goes part by part: the same bytes."""
    from test_ensembles import took_the_grouped_launch
    c = make_ctx(None, max_frames=64)
    try:
        c.set_timing(True)
        fib, ok, outs, hout = _ragged(c, 16)
        assert took_the_grouped_launch(c)
        fib4, ok4, outs4, hout4 = _ragged(c, 4)
    finally:
        c.close()
    for k in P.PROFILES:
        mother, d = P.ref(k)
        got = outs[k].reshape(4, 16, -1)
        assert (got == got[0]).all(), "the four copies of a codeword differ, " + P.name(k)
        R.assert_decoder(got[0], mother, d, True, "decode_ensembles_dev, " + P.name(k))
        assert (outs4[k] == got[0]).all(), "4 frames a stream, " + P.name(k)
        assert (hout[k] == P.history(k)).all() and (hout4[k] == P.history(k)).all(), P.name(k)
    for s in range(9):
        ref = P.fic_ref(s)
        f = fib[16 * s:16 * s + 16].reshape(4, 4, 12, 32)
        assert (f == f[0]).all()
        _assert_fic(f[0], ok[16 * s:16 * s + 4], ref, "decode_ensembles_dev, stream %d" % s)
        assert (ok[16 * s:16 * s + 16].reshape(4, 4, 12) == ref.crc_ok.reshape(4, 12)[None]).all()
        assert (fib4[4 * s:4 * s + 4] == f[0]).all() and (ok4[4 * s:4 * s + 4] == ref.crc_ok.reshape(4, 12)).all()


@pytest.fixture(scope="module")
def ber_ctx(built):
    c = make_ctx(None)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("s", range(9))
def test_gpu_channel_ber_of_every_profile(ber_ctx, s):
    """dabgpu_channel_ber_dev's own re-encoder and its reading of d_punct_idx: the sweep's soft bits and history with
    RANDOM "decoded" bytes, errors and bits of every codeword equal to quality_reference.msc_ber.  A stream's list is one
    call, which the library takes in packs of at most 16."""
    import dabgpu
    import torch
    dev = torch.device("cuda", 0)
    keys = [k for k, _ in P.streams()[s]]
    frames = P.stream_frames(s)
    d_soft = _to_dev(frames)
    d_dec = [_to_dev(P.ber_bytes(k)) for k in keys]
    d_hist = [_to_dev(P.history(k)) for k in keys]
    d_msc = [torch.full((16, 8), 0xA5, dtype=torch.uint8, device=dev) for _ in keys]
    ber_ctx.channel_ber_dev(d_soft.data_ptr(), FB, 1, 4, None, None, [_sc(k) for k in keys], [h.data_ptr() for h in d_hist],
                            [x.data_ptr() for x in d_dec], [m.data_ptr() for m in d_msc])
    ber_ctx.sync()
    for k, m in zip(keys, d_msc):
        got = m.cpu().numpy().reshape(-1).view(dabgpu.BER_DTYPE)
        p = P.profile(k)
        e, b = QR.msc_ber(frames, P.place(k)[2], p, P.ber_bytes(k), P.history(k))
        assert (got["errors"] == e).all() and (got["bits"] == b).all(), P.name(k)
        assert b.max() <= p.kept and b.min() > 0.9 * p.kept and e.min() > 0
