"""A multiplex with one DAB+ and one DAB (MPEG layer II) service, each sending its own label and one small slide in its PAD:
what synth.ServiceEnsemble's opt-in argument transmits (CPU, through the host twins), and IQ -> front end ->
dabgpu_decode_ensembles_dev -> dabgpu_dabplus_follow_dev and dabgpu_mp2_follow_dev -> dabgpu_pad_labels_dev and
dabgpu_mot_slides_dev over both kinds of rows in ONE call each (GPU)."""
import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import mp2_reference as M
from test_pad_slides import FILL, NO_PAD, image, obj

SEED = 1
SERVICES = [("Radio One", 0xC221, 3, 0, 3, 64, 0)]
DAB = [("Classic", 0xC332, 11, 17, 100)]                               # UEP index 17: 64 kbit/s, protection level 2
LABELS = ["Now: Ω Quartet – Blue in Green".encode("utf-8"), "Sinfonie Nr. 5 – Allegro con brio".encode("utf-8")]
NAMES = [b"cover-0817.jpg", b"orchestra.jpg"]
OBJECTS = [obj(0x1000, image(300, 200), NAMES[0], 128), obj(0x2000, image(900, 201), NAMES[1], 128)]
MP2_PAD_ROOM = 180                                                     # (pack_pads: an access unit of this size; the X-PAD stays below x = 182)


def dabplus_bodies():
    plain = synth.ServiceEnsemble(SEED, SERVICES, n_frames=5, dab_services=DAB, extras=False)
    sizes = [len(a) for q in plain.aus[0] for a in q]
    pads, left = synth.pack_pads(sizes, OBJECTS[0][2], synth.dls_segments(LABELS[0], 0))
    assert left == 0, "the cycle has no room for slide and label"
    return [[[synth.au_body(p) if p is not None else NO_PAD for p in pads[3 * q:3 * q + 3]] for q in range(4)]], plain


def mp2_pads():
    pads, left = synth.pack_pads([MP2_PAD_ROOM] * 20, OBJECTS[1][2], synth.dls_segments(LABELS[1], 1))
    assert left == 0 and max(len(p) for p in pads if p is not None) - 2 <= 182
    return pads


def ensemble():
    bodies, plain = dabplus_bodies()
    return synth.ServiceEnsemble(SEED, SERVICES, n_frames=5, dab_services=DAB, extras=False, bodies=bodies, dab_pads=[mp2_pads()]), plain, bodies


def test_the_opt_in_changes_nothing_else(built):
    """the default draws stay byte-identical: without dab_pads (or with None for the service) the multiplex is what it was;
    with it, only the layer-II sub-channel's capacity units differ"""
    ens, plain, bodies = ensemble()
    same = synth.ServiceEnsemble(SEED, SERVICES, n_frames=5, dab_services=DAB, extras=False, dab_pads=[None])
    assert (same.frame_bits == plain.frame_bits).all() and (same.mp2_frames[0] == plain.mp2_frames[0]).all()
    with_bodies = synth.ServiceEnsemble(SEED, SERVICES, n_frames=5, dab_services=DAB, extras=False, bodies=bodies)
    differ = np.flatnonzero((ens.frame_bits != with_bodies.frame_bits).any(axis=0)) - synth.NB_FIC_BITS
    size_cu = synth.uep_mask(17)[1]
    assert len(differ) and (differ % synth.NB_CIF_BITS >= 100 * 64).all() and (differ % synth.NB_CIF_BITS < (100 + size_cu) * 64).all()
    assert (plain.mp2_frames[0][:, 1] == 0xFD).all() and (ens.mp2_frames[0][:, 1] == 0xFC).all()


def test_the_multiplex_carries_the_layer_two_label_and_slide(built):
    """what the GPU test will receive: the transmitted layer-II frames through the host twin and the host walks"""
    from test_mp2_follow import HostMemory, call, compare, slide_of, walk_rows
    ens, plain, _b = ensemble()
    frames = np.concatenate([ens.mp2_frames[0]] * 2)                  # two cycles: the label's last segment wraps
    rc, (out,) = call(HostMemory(), [dict(B=64, frames=frames)], len(frames))
    compare(out, M.follow(list(frames), 64), "e2e")
    lab, res, slides, mres = walk_rows(out["rows"], out["status"], out["follow"][:32], len(frames) + 1)
    assert rc == 0 and dabgpu.pad_label_utf8(lab) == LABELS[1].decode("utf-8") and int(res["pad_malformed"]) == 0
    assert int(mres["slides_written"]) == 1 and slide_of(slides[0]) == OBJECTS[1][:2] and int(mres["groups_crc_failed"]) == 0
    # the frames of the multiplex as it was: header-valid only for a bit-rate index that names 64, never a row with PAD
    frames = plain.mp2_frames[0]
    rc, (out,) = call(HostMemory(), [dict(B=64, frames=frames)], len(frames))
    want = M.follow(list(frames), 64)
    compare(out, want, "plain")
    named = int(((frames[:, 2] >> 4) == 4).sum())
    assert want["result"][7] == named and (want["status"][:, 4] == 0).all()


@pytest.fixture(scope="module")
def ectx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.gpu
def test_gpu_end_to_end_iq_to_labels_and_slides_of_both_kinds(ectx):
    """three calls of 16 frames, the records swapped, the arenas in place: both labels and both slides as sent, each slide
    once.  The run without the layer-II entry is a second pair of PAD and slideshow calls in the same run, whose tables hold
    the DAB+ entry alone, with state records, arena, slots and counters of their own; they read the same rows of the one DAB+
    follow call (which never had a layer-II entry).  The DAB+ service's labels, slides, counters, state records and arena
    are byte for byte the same in both"""
    import torch
    dev = torch.device("cuda", 0)
    fps, n_calls, L, FB = 16, 3, 76 * 2552, dabgpu.NB_FRAME_BITS
    ens, _plain, _b = ensemble()
    tx = ens.iq()
    rng = np.random.default_rng(12)
    c = ectx
    c.streams_reset(1)
    n_cifs, max_sf, nb, mb = 4 * fps, (4 * fps + 4) // 5, dabgpu.pad_state_bytes(), dabgpu.mot_state_bytes()
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)
    # [0]: the tables with both entries; [1]: the DAB+ entry alone
    labels = [zeros(2, 144), zeros(1, 144)]
    slots = [torch.full((n_calls, 2, 2, 2048), FILL, dtype=torch.uint8, device=dev), torch.full((n_calls, 1, 2, 2048), FILL, dtype=torch.uint8, device=dev)]
    results, presults = [zeros(n_calls, 2, 128), zeros(n_calls, 1, 128)], [zeros(n_calls, 2, 64), zeros(n_calls, 1, 64)]
    mp2_results = zeros(n_calls, 64)
    plans = None
    for call_no in range(n_calls):
        idx = (np.arange(fps) + call_no * fps) % 5
        rx = synth.channel(tx[idx].ravel(), snr_db=20.0, rng=rng).reshape(fps, -1)
        d_iq = torch.from_numpy(np.ascontiguousarray(rx[:, synth.NB_NULL:synth.NB_NULL + L]).astype(np.complex64)).to(dev)
        d_soft = torch.zeros((fps, FB), dtype=torch.int8, device=dev)
        c.ofdm_demod_streams_dev(d_iq.data_ptr(), L, 1, fps, 0.9, d_soft.data_ptr(), None, None)
        fib, ok = zeros(fps, 12, 32), zeros(fps, 12)
        if plans is None:
            c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), [[]], None, None, None, None)
            c.sync()
            fib_h, ok_h = fib.cpu().numpy(), ok.cpu().numpy()
            assert ok_h.all()
            plans = [dabgpu.fig_subchannels(fib_h, ok_h)]
            comps = dabgpu.fig_audio_components(fib_h, ok_h)
            assert [cp.ascty for cp in comps] == [dabgpu.ASCTY_DABPLUS, dabgpu.ASCTY_DAB] and [sc.bitrate_kbps for sc in plans[0]] == [64, 64]
            hist = [[[torch.zeros((15, sc.length * 64), dtype=torch.int8, device=dev) for sc in plans[0]]] for _ in range(2)]
            carry = [[zeros(dabgpu.dabplus_carry_bytes(64)), zeros(dabgpu.mp2_carry_bytes(64))] for _ in range(2)]
            # [table][swap][entry]
            state = [[[zeros(nb) for _e in range(2 - t)] for _ in range(2)] for t in range(2)]
            mstate = [[[zeros(mb) for _e in range(2 - t)] for _ in range(2)] for t in range(2)]
            arenas = [[zeros(dabgpu.mot_arena_bytes(1024)) for _e in range(2 - t)] for t in range(2)]
        outs = [[zeros(n_cifs, 192) for _sc in plans[0]]]
        ptrs = lambda lsts: [[x.data_ptr() for x in lst] for lst in lsts]
        c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), plans, ptrs(hist[0]) if call_no else None,
                               ptrs(hist[1]), ptrs(outs), None)
        # the DAB+ entry's rows, and the layer-II entry's
        data, st, res = zeros(max_sf, 880), zeros(max_sf * 64), zeros(32)
        rows, rst, rfo = zeros(n_cifs + 1, 220), zeros((n_cifs + 1) * 64), zeros(32)
        c.dabplus_follow_dev([dabgpu.DabplusEntry(outs[0][0].data_ptr(), 192, 64, carry[0][0].data_ptr() if call_no else None,
                                                  carry[1][0].data_ptr(), data.data_ptr(), st.data_ptr(), res.data_ptr())], n_cifs)
        c.mp2_follow_dev([dabgpu.Mp2Entry(outs[0][1].data_ptr(), 192, 64, carry[0][1].data_ptr() if call_no else None, carry[1][1].data_ptr(),
                                          rows.data_ptr(), rst.data_ptr(), rfo.data_ptr(), mp2_results[call_no].data_ptr())], n_cifs)
        source = [(data.data_ptr(), 880, st.data_ptr(), res.data_ptr(), 64, max_sf),
                  (rows.data_ptr(), dabgpu.MP2_ROW_BYTES, rst.data_ptr(), rfo.data_ptr(), dabgpu.MP2_PAD_KBPS, n_cifs + 1)]
        for t in range(2):                                           # behind the follow calls on the same stream: nothing waits in between
            n_e = 2 - t
            c.mot_slides_dev([dabgpu.MotEntry(*source[j], mstate[t][0][j].data_ptr() if call_no else None, mstate[t][1][j].data_ptr(),
                                              arenas[t][j].data_ptr(), arenas[t][j].numel(), slots[t][call_no, j].data_ptr(), 2048, 2, 0,
                                              results[t][call_no, j].data_ptr()) for j in range(n_e)])
            c.pad_labels_dev([dabgpu.PadEntry(*source[j], state[t][0][j].data_ptr() if call_no else None, state[t][1][j].data_ptr(),
                                              labels[t][j].data_ptr(), presults[t][call_no, j].data_ptr()) for j in range(n_e)])
        c.sync()
        for lst in (hist, carry, state[0], state[1], mstate[0], mstate[1]):
            lst.reverse()
    got = labels[0].cpu().numpy().view(dabgpu.PAD_LABEL_DTYPE).reshape(2)
    counts = results[0].cpu().numpy().view(dabgpu.MOT_RESULT_DTYPE).reshape(n_calls, 2)
    raw = slots[0].cpu().numpy()
    mp2 = mp2_results.cpu().numpy().view(dabgpu.MP2_RESULT_DTYPE).reshape(n_calls)
    # the de-interleaver has its 16 CIFs of every frame from row 15 of the first call on: from there every frame is good
    assert mp2["id"].tolist() == [1, 1, 1] and mp2["frames"].tolist() == [64, 64, 64] and mp2["mode"].tolist() == [0, 0, 0], mp2
    bad = mp2["header_errors"] + mp2["crc_failed"] + mp2["frames_no_crc"]
    assert bad[0] <= 15 and bad[1:].tolist() == [0, 0] and mp2["synced"].tolist() == [1, 1, 1] and mp2["dropped"].sum() == 0, mp2
    for j in range(2):
        assert dabgpu.pad_label_utf8(got[j]) == LABELS[j].decode("utf-8"), j
        assert counts[:, j]["slides_written"].sum() == 1 and counts[:, j]["groups_crc_failed"].sum() == 0, counts[:, j]
        assert counts[:, j]["groups_repeated"].sum() >= len(OBJECTS[j][2])
        k = int(np.flatnonzero(counts[:, j]["slides_written"])[0])
        header, body = OBJECTS[j][0], OBJECTS[j][1]
        rec = raw[k, j, 0, :32].copy().view(dabgpu.MOT_SLIDE_DTYPE)
        assert (int(rec["transport_id"][0]), int(rec["content_type"][0]), int(rec["header_bytes"][0]), int(rec["body_bytes"][0])) == (0x1000 * (j + 1), 2, len(header), len(body))
        assert raw[k, j, 0, 32:32 + len(header)].tobytes() == header and raw[k, j, 0, 32 + len(header):32 + len(header) + len(body)].tobytes() == body
        assert dabgpu.mot_header_parse(header)["name"] == NAMES[j] and (raw[k, j, 1] == FILL).all()
    # the DAB+ entry in the table of two ([0]) and in the table of its own ([1]): labels, slots, counters, state records, arena
    for with_mp2, alone in (labels, slots, results, presults):
        a, b = with_mp2.cpu().numpy(), alone.cpu().numpy()
        assert (a[0] == b[0]).all() if a.ndim == 2 else (a[:, 0] == b[:, 0]).all()
    for with_mp2, alone in (state, mstate):
        assert all((with_mp2[side][0] == alone[side][0]).all().item() for side in range(2))
    assert (arenas[0][0] == arenas[1][0]).all().item()
