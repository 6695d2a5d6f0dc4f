"""The host mirror's layer-II channel: Basic_DAB_Channel::Process runs the shared header (include/dabgpu_mp2_frame.h) and
the existing walks, so GetDynamicLabel() and the slideshow manager work for a layer-II service exactly as for DAB+
(/root/reference/src/render_radio_block.cpp:439-486) -- with no new ABI symbol under the mirror -- and the header-only
frames the synthetic multiplex has always sent give the counts they gave.  Two levels: the channel on its own, fed logical
frames (tests/mp2_mirror_check.cpp), and the mirror as a whole -- dab_host_demo over the TEST-ONLY fake ABI of tests/fake_abi
-- from IQ through OFDM_Demod, BasicRadio and the FIC that creates the channel to GetDynamicLabel() and the slideshow manager."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dabgpu import synth

import test_mp2_end_to_end as E

HOST = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mirror") / "mp2_mirror_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mp2_mirror_check.cpp"), "-o", exe])

    def run(bitrate, frames, path):
        np.ascontiguousarray(frames, np.uint8).tofile(path)
        r = subprocess.run([exe, str(bitrate), str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        counts = {k: int(v) for k, v in (kv.split("=") for kv in lines[0].split())}
        slides = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines[2:]]
        return counts, bytes.fromhex(lines[1].split("=")[1]), slides
    return run


def test_mirror_runs_the_shared_code_and_needs_no_new_abi_symbol():
    hdr = open(os.path.join(HOST, "basic_radio", "basic_dab_channel.h")).read()
    code = "\n".join(l.split("//")[0] for l in hdr.splitlines())
    assert '#include "dabgpu_mp2_frame.h"' in code and "mp2::parse_frame(" in code and "mp2::row_byte(" in code
    assert "dabgpu_mp2_follow" not in code and "dabgpu_pad_labels" not in code and "dabgpu_mot_slides" not in code
    reader = open(os.path.join(HOST, "basic_radio", "basic_pad_reader.h")).read()
    assert "dabgpu_pad::walk_au(" in reader and "dabgpu_mot::walk_au(" in reader
    fake = open(os.path.join(ROOT, "tests", "fake_abi", "fake_dabgpu.cpp")).read()
    assert "dabgpu_mp2" not in fake                                  # the fake ABI under the mirror needs nothing new


def test_layer_two_channel_shows_its_label_and_slide(mirror, tmp_path):
    ens, _plain, _b = E.ensemble()
    frames = np.concatenate([ens.mp2_frames[0]] * 2)
    counts, label, slides = mirror(64, frames, tmp_path / "frames.bin")
    assert counts == dict(counts, frames=40, header_errors=0, is_error=0, rate=48000, kbps=64, stereo=1, checked=40, crc_errors=0, no_crc=0,
                          charset=15, new_slides=1), counts
    assert label == E.LABELS[1]
    assert len(slides) == 1 and slides[0]["name"] == E.NAMES[1].decode() and int(slides[0]["id"]) == 0x2000
    assert bytes.fromhex(slides[0]["image"]) == E.OBJECTS[1][1]
    # a frame damaged in its allocation is one lost access unit: counted, and the label still comes (it is sent again)
    bad = frames.copy()
    bad[3, 7] ^= 0x10
    counts, label, _s = mirror(64, bad, tmp_path / "bad.bin")
    assert counts["checked"] == 39 and counts["crc_errors"] == 1 and counts["header_errors"] == 0 and label == E.LABELS[1]


def test_24_khz_frames_pair_in_the_mirror(mirror, tmp_path):
    import test_mp2_follow as T
    rng = np.random.default_rng(24)
    pads, header = T.label_and_slide_pads(40)
    frames = T.audio(rng, 64, 40, T.JOINT, 1, lsf=True, pads=pads)
    for start, good in ((0, 40), (1, 39)):                               # in phase, and from a second half on
        counts, label, slides = mirror(64, frames[start:], tmp_path / ("low%d.bin" % start))
        assert counts["checked"] == good and counts["crc_errors"] == 0 and counts["rate"] == 24000, counts
        assert label == T.LABEL                                          # (sent four times)
        if start == 0:                                                   # (the slide is sent once: its first frame is needed)
            assert len(slides) == 1 and bytes.fromhex(slides[0]["image"]) == T.SLIDE
    # a lost logical frame: the first half that waited is an orphan, the next frame pairs again
    counts, label, _s = mirror(64, np.delete(frames, 5, axis=0), tmp_path / "gap.bin")
    assert counts["checked"] == 39 and counts["crc_errors"] == 0


def test_header_only_frames_count_as_they_did(mirror, tmp_path):
    """the frames the synthetic multiplex has always sent (protection bit 1, a random bit-rate index): every one a frame, no
    header error, the audio parameters of the last one, no label, no slide"""
    _ens, plain, _b = E.ensemble()
    frames = plain.mp2_frames[0]
    counts, label, slides = mirror(64, frames, tmp_path / "plain.bin")
    v1 = [0, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 0]
    assert counts["frames"] == len(frames) and counts["header_errors"] == 0 and counts["is_error"] == 0
    assert counts["rate"] == 48000 and counts["stereo"] == 1 and counts["kbps"] == v1[frames[-1, 2] >> 4]
    assert counts["checked"] == 0 and counts["crc_errors"] == 0 and counts["no_crc"] == int(((frames[:, 2] >> 4) == 4).sum())
    assert label == b"" and slides == [] and counts["new_slides"] == 0
    noise = np.random.default_rng(3).integers(0, 256, (30, 192), dtype=np.uint8)
    counts, label, slides = mirror(64, noise, tmp_path / "noise.bin")
    assert counts["frames"] == 30 and counts["header_errors"] == 30 and counts["is_error"] == 1 and label == b"" and slides == []


# ---- the mirror as a whole, over the fake ABI
@pytest.fixture(scope="module")
def demo_over_fake_abi(built, tmp_path_factory):
    """dab_host_demo and the mirror's sources linked against tests/fake_abi/fake_dabgpu.cpp (the oracle behind the mirror; never
    shipped) -> run(ensemble, directory) -> the lines of the demo's .db file"""
    fake, oracle = os.path.join(ROOT, "tests", "fake_abi"), os.path.join(ROOT, "oracle")
    exe = str(tmp_path_factory.mktemp("demo") / "dab_host_demo_fake")
    srcs = [os.path.join(HOST, "demo", "dab_host_demo.cpp"), os.path.join(fake, "fake_dabgpu.cpp")]
    srcs += [os.path.join(HOST, s) for s in ("ofdm/ofdm_demodulator.cpp", "basic_radio/basic_radio.cpp", "basic_radio/basic_dab_plus_channel.cpp", "dab/fic/fic_parser.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), "-I" + oracle, "-I" + fake] + srcs +
                          ["-L" + oracle, "-loracle", "-Wl,-rpath," + oracle, "-o", exe])

    def run(ens, where, cycles=3):
        iq = np.tile(ens.iq().ravel(), cycles)
        iq = synth.channel(iq, snr_db=20.0, cfo=0.4 / 2048, rng=np.random.default_rng(21))
        path = where / "iq.cf32"
        np.concatenate([iq[-30000:], iq, iq[:synth.NB_NULL + 5000]]).astype(np.complex64).tofile(path)
        prefix = str(where / "out")
        r = subprocess.run([exe, str(path), prefix, "40000"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "frames_desync=0" in r.stdout, r.stdout + r.stderr
        lines = open(prefix + ".db").read().splitlines()
        fields = lambda start: [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith(start)]
        return fields("channel"), fields("slide ")
    return run


def test_mirror_over_the_fake_abi_shows_label_and_slide_of_both_kinds(demo_over_fake_abi, tmp_path):
    """IQ of the multiplex of test_mp2_end_to_end.py (one DAB+ and one layer-II service, each with its own label and slide)
    -> OFDM_Demod -> BasicRadio::Process -> the channels the FIC creates, data control on: both channels show their label
    and their slide, name and image as sent"""
    ens, _plain, _b = E.ensemble()
    chans, slides = demo_over_fake_abi(ens, tmp_path)
    assert [int(c["subchannel"]) for c in chans] == [3, 11] and [int(sl["subchannel"]) for sl in slides] == [3, 11]
    assert "superframes" in chans[0] and "mp2_frames" in chans[1]
    for j, (ch, sl) in enumerate(zip(chans, slides)):
        assert bytes.fromhex(ch["label"]) == E.LABELS[j] and ch["label_charset"] == "15", ch
        assert int(sl["tid"]) == 0x1000 * (j + 1) and bytes.fromhex(sl["name"]) == E.NAMES[j], sl
        assert int(sl["bytes"]) == len(E.OBJECTS[j][1]) and bytes.fromhex(sl["body"]) == E.OBJECTS[j][1]
    mp2, n_lf = chans[1], 4 * 5 * 3 - 15                              # logical frames the de-interleaver completes
    assert n_lf - 8 <= int(mp2["mp2_frames"]) <= n_lf and mp2["header_errors"] == "0" and mp2["crc_errors"] == "0", mp2
    assert int(mp2["checked_frames"]) == int(mp2["mp2_frames"]) and (mp2["rate"], mp2["stereo"]) == ("48000", "1")


def test_mirror_over_the_fake_abi_counts_header_only_frames_as_it_did(demo_over_fake_abi, tmp_path):
    """the multiplex as it has always been sent (layer-II frames with protection bit 1 and a random bit-rate index), on the
    same path: every frame counted, no header error, 48 kHz stereo -- and no checked frame, no label, no slide"""
    _ens, plain, _b = E.ensemble()
    chans, slides = demo_over_fake_abi(plain, tmp_path)
    assert [int(c["subchannel"]) for c in chans] == [3, 11] and slides == []
    mp2, n_lf = chans[1], 4 * 5 * 3 - 15
    assert n_lf - 8 <= int(mp2["mp2_frames"]) <= n_lf and mp2["header_errors"] == "0", mp2
    assert (mp2["rate"], mp2["stereo"], mp2["checked_frames"], mp2["crc_errors"], mp2["label"]) == ("48000", "1", "0", "0", ""), mp2
