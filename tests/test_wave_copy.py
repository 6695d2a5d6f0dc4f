"""csrc/wave_copy.hpp (the whole-wave copy of mot_kernels.hip) off the device: tests/wave_copy_exhaustive.cpp under
AddressSanitizer and UBSan, every phase pair and every length, and the mutants of tests/wave_copy_mutants.py, each of which
the same program must refuse.  Stand-alone programs of the host compiler, run as child processes; nothing here needs a GPU."""
import os
import subprocess

import pytest

import wave_copy_mutants as WM
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "csrc")
SANITIZE = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fno-strict-aliasing", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all", "-I" + CSRC]


def build_exhaustive(tmp_path, k=0):
    exe = str(tmp_path / ("wave_copy_exhaustive_%d" % k))
    extra = WM.write_mutant(k, tmp_path) if k else []
    subprocess.check_call(SANITIZE + extra + [os.path.join(ROOT, "tests", "wave_copy_exhaustive.cpp"), "-o", exe])
    return exe


def test_kernel_includes_the_header_it_is_tested_by():
    src = open(os.path.join(CSRC, "mot_kernels.hip")).read()
    assert '#include "wave_copy.hpp"' in src and "wave_copy_as" not in src and src.count("wave_copy(") == 2
    assert "wave_copy.hpp" in open(os.path.join(CSRC, "Makefile")).read()


def test_exhaustive_under_sanitizers(tmp_path):
    """256 phase pairs x 1105 lengths x 3 waves each, every block exactly sized: about 8 s of one CPU core"""
    r = subprocess.run([build_exhaustive(tmp_path)], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and "phases=256 lens=1105 copies=%d " % (256 * 1105 * 3) in r.stdout, (r.stdout + r.stderr)[-4000:]


@pytest.mark.parametrize("k", sorted(WM.MUTANTS))
def test_exhaustive_refuses_every_mutant(tmp_path, k):
    """each mutant ends the program with an error -- a sanitizer's or its own; one that passes means the program is too
    weak.  (Mutant 1 is the header's equal inside the copy's contract, see wave_copy_mutants.EQUIVALENT: it must pass.)"""
    r = subprocess.run([build_exhaustive(tmp_path, k)], capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-1500:]
    print(WM.MUTANTS[k][0], "-> exit", r.returncode, "\n", "\n".join(tail.splitlines()[:6]))
    if k in WM.EQUIVALENT:
        assert r.returncode == 0 and "copies=" in r.stdout, tail
    else:
        assert r.returncode != 0 and "copies=" not in r.stdout, "mutant %d (%s) passed" % (k, WM.MUTANTS[k][0])
        assert "FAILED: " in r.stdout or "AddressSanitizer" in r.stderr or "runtime error" in r.stderr, tail
