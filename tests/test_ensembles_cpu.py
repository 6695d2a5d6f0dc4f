"""Ensembles that each have their own multiplex, without a GPU: the two entry points are exported, dabgpu_fig_subchannels
reads every ensemble's own list out of its FIBs (expected lists from the ensemble objects, the profile tables of
tests/decoder_reference.py through tests/transmit_reference.py, and oracle/fig_oracle.py), and the kernels of the ragged
grouped launch neither spill nor use scratch memory (the compiler's metadata, read as tests/test_device_asm.py reads it)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth
from oracle import fig_oracle

import decoder_reference as D
import transmit_reference as T
from conftest import ROOT
from test_device_asm import CSRC, kernel_metadata

CAPACITY, PROFILE = -6, -5

#: (services, dab_services) of three multiplexes that differ in every respect: number of sub-channels, start addresses,
#: sizes, EEP-A / EEP-B / UEP.  Deliberately NOT in start-address order.
ORGANISATIONS = [
    ([("Alpha", 0xC001, 1, 0, 3, 64, 100), ("Beta", 0xC002, 2, 1, 2, 32, 0)], [("Gamma", 0xC003, 3, 17, 30)]),
    ([("Delta", 0xC101, 9, 0, 1, 8, 700), ("Eps", 0xC102, 4, 0, 4, 48, 40), ("Zeta", 0xC103, 7, 1, 4, 64, 300),
      ("Eta", 0xC104, 5, 0, 2, 8, 0)], []),
    ([], [("Theta", 0xC201, 11, 0, 500), ("Iota", 0xC202, 12, 33, 20)]),
]


@pytest.fixture(scope="module")
def ensembles(built):
    return [synth.ServiceEnsemble(seed=40 + k, services=sv, dab_services=dab, n_frames=5, extras=False)
            for k, (sv, dab) in enumerate(ORGANISATIONS)]


def announced(e):
    """the ensemble's own list, by start address, as the tuples of dabgpu.Subchannel's fields"""
    want = []
    for (_lab, _sid, _scid, option, level, bitrate, start) in e.services:
        want.append((start, D.eep_profile(option, level, bitrate).size_cu, 0, option, level, bitrate))
    for (_lab, _sid, _scid, index, start) in e.dab_services:
        row = T.uep_rows()[index]
        want.append((start, row.size_cu, 1, 0, row.level, row.bitrate))
    return sorted(want)


def fields(scs):
    return [(s.start_address, s.length, s.is_uep, s.eep_type, s.protection_level, s.bitrate_kbps) for s in scs]


def test_both_entry_points_are_exported(built):
    L = dabgpu.lib()
    for name in ("dabgpu_decode_ensembles_dev", "dabgpu_fig_subchannels"):
        assert name in dabgpu.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.dabgpu_abi_version() == 6 == dabgpu.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    assert "#define DABGPU_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", hdr)


def test_fig_subchannels_returns_each_ensembles_own_list(ensembles):
    ok = np.ones((5, 12), np.uint8)
    lists = []
    for e in ensembles:
        got = fields(dabgpu.fig_subchannels(e.fibs, ok))
        assert got == announced(e)
        # ... and what the FIG oracle reads from the same FIBs agrees, field by field (it does not restate the UEP sizes)
        db = fig_oracle.parse_fibs(e.fibs.reshape(-1, 32))
        by_start = sorted(db.subchannels.values(), key=lambda s: s["start_address"])
        assert len(by_start) == len(got)
        for o, g in zip(by_start, got):
            assert o["start_address"] == g[0] and int(o["is_uep"]) == g[2]
            if o["is_uep"]:
                assert T.uep_rows()[o["uep_prot_index"]].size_cu == g[1]
            else:
                assert (o["length"], o["eep_type"], o["eep_prot_level"] + 1) == (g[1], g[3], g[4])
        lists.append(got)
    assert lists[0] != lists[1] != lists[2] != lists[0]
    # the short form gives the UEP row; both EEP options come back
    row = T.uep_rows()[17]
    assert lists[0][1] == (30, row.size_cu, 1, 0, row.level, row.bitrate) == tuple(fields([dabgpu.uep_subchannel(17, 30)])[0])
    assert {g[3] for g in lists[0] if not g[2]} == {0, 1} and {g[3] for g in lists[1]} == {0, 1}
    assert all(g[2] == 1 for g in lists[2])


def test_fig_subchannels_lists_a_repeated_sub_channel_once(ensembles):
    e = ensembles[1]
    ok = np.ones((5, 12), np.uint8)
    # every CIF of every frame repeats FIG 0/1: 20 announcements of each sub-channel, one entry each
    one = fields(dabgpu.fig_subchannels(e.fibs[:1], ok[:1]))
    assert one == fields(dabgpu.fig_subchannels(e.fibs, ok)) == announced(e) and len(one) == 4
    assert fields(dabgpu.fig_subchannels(np.concatenate([e.fibs, e.fibs]), np.concatenate([ok, ok]))) == announced(e)


def test_fig_subchannels_ignores_fibs_whose_crc_failed(ensembles):
    a, b = ensembles[0], ensembles[1]
    # b's FIBs marked bad among a's: only a's list; everything marked bad: nothing
    fibs = np.concatenate([b.fibs, a.fibs])
    ok = np.concatenate([np.zeros((5, 12), np.uint8), np.ones((5, 12), np.uint8)])
    assert fields(dabgpu.fig_subchannels(fibs, ok)) == announced(a)
    assert dabgpu.fig_subchannels(a.fibs, np.zeros((5, 12), np.uint8)) == []
    # only the FIB that carries FIG 0/1 marked bad, in every CIF: nothing is found either
    carries = np.array([[len(fig_oracle.parse_fibs([a.fibs[f, k]]).subchannels) > 0 for k in range(12)] for f in range(5)])
    assert carries.any() and not carries.all()
    assert dabgpu.fig_subchannels(a.fibs, (~carries).astype(np.uint8)) == []
    assert fields(dabgpu.fig_subchannels(a.fibs, carries.astype(np.uint8))) == announced(a)


def test_fig_subchannels_capacity_and_profile_errors(ensembles):
    e = ensembles[1]
    ok = np.ones((5, 12), np.uint8)
    L = dabgpu.lib()
    arr = (dabgpu.Subchannel * 4)()
    n = C.c_int(-1)
    fib = np.ascontiguousarray(e.fibs)
    assert L.dabgpu_fig_subchannels(fib.ctypes.data, ok.ctypes.data, 5, arr, 3, C.byref(n)) == CAPACITY and n.value == 4
    assert L.dabgpu_fig_subchannels(fib.ctypes.data, ok.ctypes.data, 5, None, 0, C.byref(n)) == CAPACITY and n.value == 4
    assert L.dabgpu_fig_subchannels(fib.ctypes.data, ok.ctypes.data, 5, arr, 4, C.byref(n)) == 0 and n.value == 4
    assert fields(arr) == announced(e)
    with pytest.raises(dabgpu.DabGpuError) as err:
        dabgpu.fig_subchannels(e.fibs, ok, max_out=2)
    assert err.value.status == CAPACITY
    # a size that is no multiple of the level's capacity units names no profile (EEP 3-A: 6 CU per 8 kbit/s)
    bad = synth.pack_fibs([synth.fig0_1([{"id": 1, "start": 0, "option": 0, "level": 3, "size": 47}])])
    with pytest.raises(dabgpu.DabGpuError) as err:
        dabgpu.fig_subchannels(np.concatenate([bad] * 12)[None], np.ones((1, 12), np.uint8))
    assert err.value.status == PROFILE
    # the next configuration (C/N = 1) is not the current one; a reserved long-form option is passed over
    nxt = synth.pack_fibs([synth.fig0(1, synth.fig0_1([{"id": 1, "start": 0, "option": 0, "level": 3, "size": 48}])[2:], cn=1),
                           synth.fig0_1([{"id": 2, "start": 100, "option": 2, "level": 3, "size": 48},
                                         {"id": 3, "start": 200, "option": 1, "level": 3, "size": 36}])])
    got = dabgpu.fig_subchannels(np.concatenate([nxt] * 12)[:12][None], np.ones((1, 12), np.uint8))
    assert fields(got) == [(200, 36, 0, 1, 3, 64)]


def test_ragged_launch_kernels_neither_spill_nor_use_scratch(built, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the device assembly cannot be checked")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    out = tmp_path / "viterbi_lane_kernels.s"
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "viterbi_lane_kernels.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    md = kernel_metadata(out.read_text())
    one = lambda part: [v for k, v in md.items() if part in k]
    fwd, tb, hist = one("lane_forward_ragged_kernel"), one("lane_traceback_ragged_kernel"), one("lane_history_ragged_kernel")
    assert len(fwd) == len(tb) == len(hist) == 1
    for v in fwd + tb + hist:
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v
    # the forward pass and the ring copy keep every scalar in a register as well, and the forward pass the occupancy of the
    # by-value grouped kernel it stands beside (two waves per SIMD)
    assert fwd[0]["sgpr_spill_count"] == 0 and hist[0]["sgpr_spill_count"] == 0
    grouped_fwd, grouped_tb = one("lane_forward_grouped_kernel")[0], one("lane_traceback_grouped_kernel")[0]
    assert fwd[0]["vgpr_count"] <= grouped_fwd["vgpr_count"] <= 256
    # the traceback body (shared, unchanged) parks scalars in vector-register lanes -- never in memory -- in every kernel
    # that runs it; the ragged kernel adds none to what the grouped kernel's count already is
    assert tb[0]["sgpr_spill_count"] <= grouped_tb["sgpr_spill_count"] and tb[0]["vgpr_count"] <= grouped_tb["vgpr_count"]
