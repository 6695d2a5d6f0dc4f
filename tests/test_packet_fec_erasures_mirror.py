"""The host mirror's data packet channel with lost packets as erasures: with FEC scheme 1 (BasicRadio switches the correction
on from FIG 0/14) Basic_Data_Packet_Channel runs process_erasures of include/dabgpu_packet_fec_erasures.h in front of its
walk -- the header directly, so no export of the library is called.  The chain stream of tests/test_packet_fec_erasures.py,
eight wiped slots in every FEC frame, goes through the channel a frame a call (tests/packet_fec_erasures_mirror_check.cpp):
the slide is the one sent and the FEC counters are tests/packet_fec_erasure_reference.py's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import packet_fec_erasure_reference as E
import test_packet as T
import test_packet_fec_erasures as X

HOST = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mirror") / "packet_fec_erasures_mirror_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "packet_fec_erasures_mirror_check.cpp"), "-o", exe])

    def run(bitrate, fec, frames, path, address):
        np.ascontiguousarray(frames, np.uint8).tofile(path)
        r = subprocess.run([exe, str(bitrate), str(fec), str(path), str(address)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        parse = lambda l: {k: int(v) for k, v in (kv.split("=") for kv in l.split())}
        return parse(lines[0]), parse(lines[1]), [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines[2:]]
    return run


def test_mirror_runs_the_erasure_header_for_scheme_1():
    hdr = open(os.path.join(HOST, "basic_radio", "basic_data_packet_channel.h")).read()
    code = "\n".join(l.split("//")[0] for l in hdr.splitlines())
    assert '#include "dabgpu_packet_fec_erasures.h"' in code and "fec::process_erasures(" in code and "m_fec == 1" in code
    assert "dabgpu_packet_fec_erasures_host" not in code and "dabgpu_packet_fec_erasures_dev" not in code
    fake = open(os.path.join(ROOT, "tests", "fake_abi", "fake_dabgpu.cpp")).read()
    assert "dabgpu_packet" not in fake


def test_channel_recovers_eight_lost_slots_per_fec_frame_and_shows_the_slide(mirror, tmp_path):
    _sent, raw = X.chain_frames()
    body = X.CHAIN_OBJECT[1]
    fec_counts, packets, slides = mirror(32, 1, raw, tmp_path / "frames.bin", T.ADDR)
    _fixed, wc = E.Receiver(32).call(raw)
    want = X.counts_of(wc)
    assert fec_counts.pop("corrects") == 1 and fec_counts.pop("same") == 1 and fec_counts == want
    assert want["frames"] == 2 and want["rows_erasure_corrected"] == 24 and want["rows_uncorrectable"] == 0 and want["slots_suspect"] == 16
    assert packets["frames"] == len(raw) and packets["slots_bad"] == 0 and packets["packets_fec"] == 18 and packets["continuity_breaks"] == 0
    assert [(int(s["id"]), bytes.fromhex(s["image"])) for s in slides] == [(0x612, body)]
    # a scheme that is not corrected loses it
    fec_counts, packets, slides = mirror(32, 2, raw, tmp_path / "frames.bin", T.ADDR)
    assert fec_counts["corrects"] == 0 and fec_counts["cifs"] == 0 and slides == [] and packets["slots_bad"] >= 8
