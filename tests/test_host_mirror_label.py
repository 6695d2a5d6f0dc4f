"""The host mirror shows the dynamic label: Basic_DAB_Plus_Channel::Process runs the walk of include/dabgpu_pad_walk.h over
the access units it already has in host memory and GetDynamicLabel() returns the current label's bytes, as the reference's
GUI prints them (/root/reference/src/render_radio_block.cpp:425-427, 470-472).  The IQ is that of
test_pad_labels.py::test_gpu_end_to_end_iq_to_labels: two DAB+ services, two labels."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dabgpu import synth

from test_pad_labels import E2E_LABELS, E2E_SEED, E2E_SERVICES, e2e_bodies

HOST = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")


def test_mirror_reads_pad_with_the_shared_walk_and_no_new_abi_symbol():
    src = open(os.path.join(HOST, "basic_radio", "basic_dab_plus_channel.cpp")).read()
    hdr = open(os.path.join(HOST, "basic_radio", "basic_dab_plus_channel.h")).read()
    assert '#include "dabgpu_pad_walk.h"' in hdr and "dabgpu_pad::walk_au(" in src
    assert "dabgpu_pad_labels" not in src + hdr and "dabgpu_pad_label_utf8" not in src + hdr
    fake = open(os.path.join(ROOT, "tests", "fake_abi", "fake_dabgpu.cpp")).read()
    assert "dabgpu_pad" not in fake                                  # the fake ABI under the mirror needs nothing new


@pytest.mark.gpu
def test_demo_shows_both_dynamic_labels(built, tmp_path):
    if not os.path.exists(os.path.join(HOST, "dab_host_demo")):
        subprocess.check_call(["make", "-C", HOST, "-j4"], stdout=subprocess.DEVNULL)
    ens = synth.ServiceEnsemble(E2E_SEED, E2E_SERVICES, n_frames=5, extras=False, bodies=e2e_bodies())
    iq = np.tile(ens.iq().ravel(), 3)
    iq = synth.channel(iq, snr_db=20.0, cfo=0.4 / 2048, rng=np.random.default_rng(21))
    path = tmp_path / "iq.cf32"
    np.concatenate([iq[-30000:], iq, iq[:synth.NB_NULL + 5000]]).astype(np.complex64).tofile(path)
    prefix = str(tmp_path / "out")
    r = subprocess.run([os.path.join(HOST, "dab_host_demo"), str(path), prefix, "40000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "frames_desync=0" in r.stdout, r.stdout + r.stderr
    chans = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in open(prefix + ".db").read().splitlines() if l.startswith("channel")]
    assert [int(c["subchannel"]) for c in chans] == [3, 7]
    for c, sent in zip(chans, E2E_LABELS):
        assert bytes.fromhex(c["label"]) == sent and c["label_charset"] == "15", c
