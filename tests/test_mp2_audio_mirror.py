"""The host mirror's layer-II channel and its audio level: Basic_DAB_Channel::GetAudioLevel() is the level record of the last
good frame, through the serial decoder of include/dabgpu_mp2_audio.h -- the record the host twin dabgpu_mp2_subbands_host
writes for the same frame (tests/mp2_audio_mirror_check.cpp feeds the channel logical frames one at a time)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import test_mp2_audio as TA

HOST = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mirror") / "mp2_audio_mirror_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mp2_audio_mirror_check.cpp"), "-o", exe])

    def run(bitrate, frames, path, audio=1, data=1):
        np.ascontiguousarray(frames, np.uint8).tofile(path)
        r = subprocess.run([exe, str(bitrate), str(path), str(audio), str(data)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return [line.split() for line in r.stdout.splitlines()]
    return run


def twin_levels(name):
    """the host twin's level records of a case's rows, and the logical frame that completes each row"""
    c = TA.CASES[name]
    rc, (out,) = TA.run(TA.Host(), [dict(c, carry=None)], 4)
    assert rc == (0, 0)
    n, phase = int(out["result"]["frames"]), int(out["result"]["phase"])
    per = 2 if c["lsf"] else 1
    return out["levels"][:32 * n].view(TA.LEVEL), [phase + per * k + per - 1 for k in range(n)]


def same(line, lv):
    got = [int(v) for v in line[:4]] + [int(v, 16) for v in line[4:8]]
    power = np.array(got[4:6], np.uint32).view(np.float32).astype(np.float64)
    want = lv["power"].astype(np.float64)
    return (got[:4] == [int(lv[f]) for f in ("kind", "channels", "cells", "scf63")] and got[6:8] == TA.bits(lv["peak"]).tolist()
            and bool((np.abs(power - want) <= TA.POWER_TOL * want).all()))


@pytest.mark.parametrize("name", ["every scale-factor index and every SCFSI", "slots that are not good", "joint stereo bound 8 48 kHz",
                                  "joint stereo bound 12 24 kHz", "the audio ends at the limit, and one bit behind it",
                                  "silent frames and frames with a PAD", "24 kHz from a second half on"])
def test_the_level_of_the_mirror_is_the_host_twin_s(built, mirror, tmp_path, name):
    c = TA.CASES[name]
    levels, done = twin_levels(name)
    lines = mirror(c["B"], c["frames"], tmp_path / "frames.bin")
    assert len(lines) == 4
    last = None
    for i, line in enumerate(lines):
        if i in done and int(levels[done.index(i)]["kind"]) != TA.A.NOT_GOOD:
            last = levels[done.index(i)]
        if last is None:
            assert line[0] == "none", (name, i, line)
        else:
            assert same(line, last), (name, i, line, last)
    assert last is not None


def test_the_level_follows_the_audio_control_and_leaves_the_counts_alone(built, mirror, tmp_path):
    c = TA.CASES["unharmed"]
    on = mirror(c["B"], c["frames"], tmp_path / "a.bin", audio=1, data=1)
    off = mirror(c["B"], c["frames"], tmp_path / "b.bin", audio=0, data=1)
    only = mirror(c["B"], c["frames"], tmp_path / "c.bin", audio=1, data=0)
    assert [l[-1] for l in on] == [l[-1] for l in off] == ["checked=%d" % k for k in (1, 2, 3, 4)]
    assert all(l[0] == "none" for l in off) and all(l[0] == "0" for l in on)
    assert [l[:8] for l in only] == [l[:8] for l in on] and [l[-1] for l in only] == ["checked=0"] * 4
