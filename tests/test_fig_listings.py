"""The five FIG listing calls (include/dabgpu.h: dabgpu_fig_subchannels, _audio_components, _packet_components, _user_applications,
_stream_components; one walker, include/dabgpu_fig.h) against what the library recorded in tests/golden/fig_listing_cases.npz
returned before they shared it (tests/golden/make_fig_listing_cases.py: the cases, and how a call is run), byte for byte; and the
header alone, under AddressSanitizer and UBSan."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from golden import make_fig_listing_cases as G


@pytest.fixture(scope="module")
def recorded():
    return G.load()


@pytest.mark.parametrize("call", list(G.CALLS))
def test_listing_returns_what_was_recorded(built, recorded, call):
    """Status, *n and every byte of the output buffer -- the entries and the fill behind them, or all of it after a refusal --
    of every recorded case at max large, exact and one too small."""
    cases, results = recorded
    meta, blob = results[call]
    assert len(cases) > 100 and meta.shape == (len(cases), 3, 3)
    at = 0
    for (name, fib, crc_ok), rows in zip(cases, meta):
        for max_out, status, n in rows:
            rc, got_n, out = G.run_call(call, fib, crc_ok, int(max_out))
            want = blob[at:at + out.size]
            at += out.size
            assert (rc, got_n) == (status, n), (name, int(max_out))
            assert np.array_equal(out, want), (name, int(max_out))
            if status != G.OK:
                assert (out == G.FILL).all(), (name, int(max_out))
    assert at == blob.size


def test_header_alone_under_sanitizers(tmp_path):
    """tests/fig_listing_fuzz.cpp: include/dabgpu_fig.h on random bytes and damaged FIBs at the end of exactly sized heap blocks."""
    exe = tmp_path / "fig_listing_fuzz"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "fig_listing_fuzz.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), "4000"], text=True)
    assert "fig_listing_fuzz ok" in out, out
