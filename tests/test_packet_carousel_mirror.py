"""The host mirror's data packet channel, its directory-mode side: Basic_Data_Packet_Channel::Process runs the control of
include/dabgpu_mot_carousel.h beside its walk on the same followed packets (tests/packet_carousel_mirror_check.cpp).  The
carousel streams of tests/test_packet_carousel.py give the objects, the current directory and the counters of
tests/carousel_reference.py; the header-mode streams of tests/test_packet.py give the slides and counters they gave before
(tests/packet_mirror_check.cpp's lines, unchanged), while the carousel control beside them counts groups_header_mode."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import carousel_reference as R
import test_packet as T
import test_packet_carousel as TC

HOST = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")
#: the channel's own sizes (Basic_Data_Packet_Channel::Carousel)
SIZES, STRIDE = (64 * 1024, 8, 256 * 1024), 32 + 8191 + 256 * 1024
KEYS = ("packets_followed", "continuity_breaks", "groups_opened", "group_bytes", "groups_ok", "groups_crc_failed", "groups_ignored_type",
        "groups_malformed", "groups_repeated", "segments_placed", "segments_early_last", "objects_completed", "objects_mismatched",
        "objects_too_large", "groups_header_mode", "groups_compressed_directory", "groups_unlisted", "directories_completed",
        "directories_mismatched", "directories_too_large", "objects_stale", "objects_evicted", "objects_dropped", "objects_deferred",
        "directory_id", "directory_bytes", "directory_objects", "directory_period")


@pytest.fixture(scope="module")
def mirrors(tmp_path_factory):
    out = {}
    for name in ("packet_carousel_mirror_check", "packet_mirror_check"):
        exe = str(tmp_path_factory.mktemp("mirror") / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe])
        out[name] = exe

    def run(which, bitrate, fec, frames, path, addresses):
        np.ascontiguousarray(frames, np.uint8).tofile(path)
        r = subprocess.run([out[which], str(bitrate), str(fec), str(path)] + [str(a) for a in addresses], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.splitlines()
    return run


def fields(line):
    return dict(kv.split("=", 1) for kv in line.split()[1:])


CAROUSEL_STREAMS = ["plain, directory in 3", "bodies first, directory out of order", "interleaved, K 4", "three cycles", "directory change", "N 256",
                    "check: trailing bytes", "other types", "body_size mismatch", "segment sizes", "header offsets of every residue", "rate 8"]


@pytest.mark.parametrize("name", CAROUSEL_STREAMS)
def test_channel_delivers_directory_and_objects_as_the_reference(mirrors, tmp_path, name):
    st = TC.streams()[name]
    lines = mirrors("packet_carousel_mirror_check", st["bitrate"], 0, st["frames"], tmp_path / "frames.bin", [TC.ADDR])
    # (slots enough for every object: the channel takes each as it is emitted, so nothing is ever deferred)
    objs, _d, res = R.Receiver(*SIZES, TC.ADDR).call(st["frames"], st["bitrate"], 64, STRIDE)
    got = fields([l for l in lines if l.startswith("carousel ")][0])
    assert {k: int(got[k]) for k in KEYS} == {k: TC.count_of(res, k) for k in KEYS}, name
    sent = [l for l in lines if l.startswith("object ")]
    assert [(int(f["id"]), int(f["type"]), int(f["subtype"]), int(f["directory"]), f["header"], f["body"]) for f in map(fields, sent)] == \
        [(int(r["transport_id"][0]), int(r["content_type"][0]), int(r["content_subtype"][0]), int(r["directory_id"][0]), h.hex(), b.hex()) for r, h, b in objs], name
    current = R.Receiver(*SIZES, TC.ADDR)
    current.call(st["frames"], st["bitrate"], 64, STRIDE)
    cur = current.mot.current
    d = fields([l for l in lines if l.startswith("directory ")][0])
    assert (int(d["bytes"]), d.get("data", "")) == ((len(cur["data"]), cur["data"].hex()) if cur else (0, "")), name
    # the header-mode walk beside it is what it was: it knows no type 6 and completes nothing from bodies alone
    assert not [l for l in lines if l.startswith("slide ")] or name == "other types"


#: the streams tests/test_packet_mirror.py holds the channel to, and "slots" (a repeated object)
@pytest.mark.parametrize("name", ["lengths", "resync", "addresses, fec 0", "addresses, fec 1", "continuity", "useful lengths", "commands", "small", "long", "slots"])
def test_the_walk_beside_the_carousel_control_is_unchanged(mirrors, tmp_path, name):
    """the existing streams: the channel's own lines (counters per address, slides) are, byte for byte, those of
    packet_mirror_check.cpp, whose counters tests/test_packet_mirror.py holds to the packet reference; the carousel control
    sees the same groups and takes none of them for its own"""
    st = T.streams()[name]
    sp = T.spec_of(st)
    args = (st["bitrate"], sp.get("fec", 0), st["frames"], tmp_path / "frames.bin", [sp.get("address", T.ADDR)])
    with_carousel, plain = mirrors("packet_carousel_mirror_check", *args), mirrors("packet_mirror_check", *args)
    assert with_carousel[:len(plain)] == plain and plain
    c = fields([l for l in with_carousel if l.startswith("carousel ")][0])
    walk = fields(plain[1])
    assert int(c["packets_followed"]) == int(walk["packets_followed"]) and int(c["group_bytes"]) == int(walk["group_bytes"])
    assert int(c["directories_completed"]) == 0 and not [l for l in with_carousel if l.startswith("object ")]
    if st["slides"]:
        assert int(c["groups_header_mode"]) > 0


def test_mirror_runs_the_shared_code():
    hdr = open(os.path.join(HOST, "basic_radio", "basic_data_packet_channel.h")).read()
    code = "\n".join(l.split("//")[0] for l in hdr.splitlines())
    assert '#include "dabgpu_mot_carousel.h"' in code and "car::walk_packet(" in code and "dabgpu_packet_carousel" not in code
