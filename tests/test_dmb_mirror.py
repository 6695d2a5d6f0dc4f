"""The host mirror's Basic_DMB_Channel (host/basic_radio/basic_dmb_channel.h) against the host twin: tests/dmb_mirror_check.cpp
feeds a damaged stream frame by frame, under AddressSanitizer and UBSan; packets, statistics and census have to be what
dabgpu_dmb_follow_host gives for the same frames in one call.  The channel calls no export of libdabgpu, so the test-only fake
ABI is neither linked nor changed."""
import os
import subprocess

import numpy as np

import dabgpu
from conftest import ROOT
from test_dmb import host_call, noisy, run_stream

HOST = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")


def test_fake_abi_has_no_dmb_symbol(built):
    assert "dmb" not in open(os.path.join(ROOT, "tests", "fake_abi", "fake_dabgpu.cpp")).read()


def test_mirror_channel_is_the_host_twin(built, tmp_path):
    exe = str(tmp_path / "dmb_mirror_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "dmb_mirror_check.cpp"), "-o", exe])
    frames = noisy(136, 60, 23)
    frames = np.concatenate([frames[:30], frames[31:]])                     # a frame is lost: two locks
    (tmp_path / "frames.bin").write_bytes(frames.tobytes())
    out = subprocess.check_output([exe, "136", str(tmp_path / "frames.bin"), str(tmp_path / "out.ts")], text=True).splitlines()
    want = run_stream(host_call, 136, frames)
    c = want["counts"]
    assert c["locks"] >= 1 and c["packets_corrected"] > 0 and c["packets_uncorrectable"] > 0 and c["packets_emitted"] > 60
    assert (tmp_path / "out.ts").read_bytes() == want["ts"].tobytes()
    stats = dict(kv.split("=") for kv in out[0].split())
    names = {"emitted": "packets_emitted", "clean": "packets_clean", "corrected": "packets_corrected", "uncorrectable": "packets_uncorrectable",
             "dropped": "packets_dropped"}
    assert {names.get(k, k): int(v) for k, v in stats.items()} == c
    assert out[1] == "handed=%d ignored=1" % c["packets_emitted"]
    census = dabgpu.dmb_state_census(want["state"], 136)
    assert out[2:] == ["pid=%d packets=%d discontinuities=%d duplicates=%d scrambled=%d" % (e["pid"], e["packets"], e["discontinuities"], e["duplicates"],
                                                                                           e["scrambled"]) for e in census]
