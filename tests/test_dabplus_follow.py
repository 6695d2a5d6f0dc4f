"""dabgpu_dabplus_follow_dev (every DAB+ sub-channel of a batch followed to super-frames on the device: alignment, carry
between calls, RS / Fire code / AU CRCs) and dabgpu_fig_audio_components (which sub-channels carry DAB+), against
tests/dabplus_follow_reference.py: data parts, status records, result records and carry records byte for byte, every
output between sentinel bytes.

CPU: exports, refusals that need no device (a NULL context: the same table errors are refused with a live context in
the GPU test of refusals), the carry size, the FIG 0/2 reader against synth.ServiceEnsemble and a from-definition walk
written here, the reference's own properties, the compiler's metadata of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import dabplus_follow_reference as F
import dabplus_reference as R
from test_device_asm import CSRC, kernel_metadata

ARG, CAPACITY = -1, -6
FB = dabgpu.NB_FRAME_BITS


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_are_exported_and_typed(built):
    L = dabgpu.lib()
    for name in ("dabgpu_dabplus_follow_dev", "dabgpu_dabplus_carry_bytes", "dabgpu_fig_audio_components"):
        assert name in dabgpu.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.dabgpu_abi_version() == 6 == dabgpu.ABI_VERSION
    assert C.sizeof(dabgpu.DabplusEntry) == 64 and dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE.itemsize == 32 == F.RESULT_DTYPE.itemsize
    assert dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE.names == F.RESULT_DTYPE.names
    assert dabgpu.AUDIO_COMPONENT_DTYPE.itemsize == 32 == C.sizeof(dabgpu.AudioComponent)
    assert hasattr(dabgpu.Context, "dabplus_follow_dev")


def test_carry_bytes(built):
    for br in range(8, 513, 8):
        assert dabgpu.dabplus_carry_bytes(br) == 16 + 4 * 3 * br == F.carry_bytes(br // 8) and dabgpu.dabplus_carry_bytes(br) % 16 == 0
    for br in (0, -8, 4, 12, 513, 520):
        assert dabgpu.dabplus_carry_bytes(br) == 0


def _entry(bitrate=64, d_in=0x10000, stride=None, cin=0x20000, cout=0x30000, data=0x40000, status=0x50000, result=0x60000):
    return dabgpu.DabplusEntry(d_in, 3 * bitrate if stride is None else stride, bitrate, cin, cout, data, status, result)


#: (what is wrong, the table) -- each refused with DABGPU_ERR_ARG before anything is enqueued
BAD_TABLES = [
    ("bit rate no multiple of 8", [_entry(), _entry(bitrate=12, stride=192)]),
    ("bit rate 0", [_entry(bitrate=0, stride=192)]),
    ("bit rate above 512", [_entry(bitrate=520)]),
    ("in_stride below bitrate * 3", [_entry(), _entry(stride=191)]),
    ("carry in == out", [_entry(cin=0x30000)]),
    ("carry in overlaps out", [_entry(cin=0x30000 - 16)]),
    ("carry off its boundary", [_entry(cout=0x30008)]),
    ("null carry out", [_entry(cout=None)]),
    ("null result", [_entry(result=None)]),
    ("null input", [_entry(d_in=None)]),
    ("null data", [_entry(data=None)]),
    ("status off its boundary", [_entry(status=0x50002)]),
]


def test_refusals_that_need_no_device(built):
    L = dabgpu.lib()
    good = (dabgpu.DabplusEntry * 1)(_entry())
    assert L.dabgpu_dabplus_follow_dev(None, good, 1, 16, None) == ARG           # no context
    for what, table in BAD_TABLES:
        arr = (dabgpu.DabplusEntry * len(table))(*table)
        assert L.dabgpu_dabplus_follow_dev(None, arr, len(table), 16, None) == ARG, what
    assert L.dabgpu_dabplus_follow_dev(None, None, 1, 16, None) == ARG           # null table
    assert L.dabgpu_dabplus_follow_dev(None, good, -1, 16, None) == ARG          # negative counts
    assert L.dabgpu_dabplus_follow_dev(None, good, 1, -1, None) == ARG


# ---- FIG 0/1 + FIG 0/2 from the definition (EN 300 401 clauses 5.2.2, 6.2.1, 6.3.1), bit by bit
def _take(bits, at, n):
    return int("".join(map(str, bits[at:at + n])), 2), at + n


def walk_audio_components(fibs, ok):
    """[(sid, subchid, start, ascty, primary)] of the MSC stream audio components, each sub-channel once, by start address"""
    starts, comps = {}, []
    for fib, good in zip(np.asarray(fibs, np.uint8).reshape(-1, 32), np.asarray(ok).reshape(-1)):
        if not good:
            continue
        i = 0
        while i < 30 and fib[i] != 0xFF:
            ftype, length = fib[i] >> 5, fib[i] & 0x1F
            if length == 0 or i + 1 + length > 30:
                break
            bits = np.unpackbits(fib[i + 1:i + 1 + length]).tolist()
            i += 1 + length
            if ftype != 0:
                continue
            cn, oe, pd = bits[0], bits[1], bits[2]
            ext, at = _take(bits, 3, 5)
            if cn or oe:
                continue
            if ext == 1:
                while at + 24 <= len(bits):
                    subch, at = _take(bits, at, 6)
                    start, at = _take(bits, at, 10)
                    long_form, at = _take(bits, at, 1)
                    if long_form:
                        option, at = _take(bits, at, 3)
                        at += 12
                        if option > 1:
                            continue
                    else:
                        at += 7
                    starts.setdefault(subch, start)
            elif ext == 2:
                while at + (32 if pd else 16) + 8 <= len(bits):
                    sid, at = _take(bits, at, 32 if pd else 16)
                    at += 4
                    ncomp, at = _take(bits, at, 4)
                    for _ in range(ncomp):
                        tmid, at = _take(bits, at, 2)
                        ascty, at = _take(bits, at, 6)
                        subch, at = _take(bits, at, 6)
                        ps, at = _take(bits, at, 1)
                        at += 1
                        if tmid == 0:
                            comps.append((sid, subch, ascty, ps))
    out, seen = [], set()
    for sid, subch, ascty, ps in comps:
        if subch in seen or subch not in starts:
            continue
        seen.add(subch)
        out.append((sid, subch, starts[subch], ascty, ps))
    return sorted(out, key=lambda c: c[2])


def comp_fields(comps):
    return [(c.sid, c.subchid, c.start_address, c.ascty, c.primary) for c in comps]


MIXED = [
    ([("Alpha", 0xC001, 1, 0, 3, 64, 100), ("Beta", 0xC002, 2, 1, 2, 32, 0)], [("Gamma", 0xC003, 3, 17, 30)]),
    ([("Delta", 0xC101, 9, 0, 1, 8, 700), ("Eps", 0xC102, 4, 0, 4, 48, 40), ("Zeta", 0xC103, 7, 1, 4, 64, 300)],
     [("Eta", 0xC104, 5, 0, 0)]),
    ([], [("Theta", 0xC201, 11, 0, 500), ("Iota", 0xC202, 12, 33, 20)]),
]


@pytest.fixture(scope="module")
def mixed(built):
    return [synth.ServiceEnsemble(seed=70 + k, services=sv, dab_services=dab, n_frames=5, extras=False)
            for k, (sv, dab) in enumerate(MIXED)]


def test_fig_audio_components_of_mixed_ensembles(mixed):
    ok = np.ones((5, 12), np.uint8)
    for e in mixed:
        want = [(sid, scid, start, 63, 1) for (_l, sid, scid, _o, _lv, _br, start) in e.services]
        want += [(sid, scid, start, 0, 1) for (_l, sid, scid, _ix, start) in e.dab_services]
        want.sort(key=lambda c: c[2])
        got = comp_fields(dabgpu.fig_audio_components(e.fibs, ok))
        assert got == want == walk_audio_components(e.fibs, ok)
        # the join: the start addresses are those of the list dabgpu_fig_subchannels returns, in the same order
        assert [g[2] for g in got] == [sc.start_address for sc in dabgpu.fig_subchannels(e.fibs, ok)]
        # one frame says it all; FIBs whose CRC failed say nothing
        assert comp_fields(dabgpu.fig_audio_components(e.fibs[:1], ok[:1])) == want
        assert dabgpu.fig_audio_components(e.fibs, np.zeros((5, 12), np.uint8)) == []
    kinds = [{g[3] for g in comp_fields(dabgpu.fig_audio_components(e.fibs, ok))} for e in mixed]
    assert kinds == [{0, 63}, {0, 63}, {0}]


def _fig0_2_raw(body, pd=0, cn=0, oe=0):
    return synth.fig0(2, body, cn=cn, oe=oe, pd=pd)


def test_fig_audio_components_forms_and_omissions(built):
    B = synth._bits
    sub = synth.fig0_1([{"id": 1, "start": 300, "option": 0, "level": 3, "size": 48}, {"id": 2, "start": 0, "uep_index": 17},
                        {"id": 3, "start": 100, "option": 1, "level": 3, "size": 36}, {"id": 9, "start": 500, "option": 2, "level": 3, "size": 48},
                        {"id": 10, "start": 600, "option": 0, "level": 3, "size": 6}])
    figs = [
        sub,
        # P/D = 1: 32-bit SId; a secondary DAB+ component beside a packet-mode one (TMId 3) and a data stream (TMId 1)
        _fig0_2_raw(B((0xE1C00123, 32), (0, 1), (0, 3), (3, 4)) + B((3, 2), (0x123, 12), (0, 1), (0, 1)) +
                    B((1, 2), (5, 6), (10, 6), (1, 1), (0, 1)) + B((0, 2), (63, 6), (3, 6), (0, 1), (0, 1)), pd=1),
        # P/D = 0: a DAB component, then sub-channel 3 again (listed once: its first component), one on a sub-channel nobody
        # announced (id 20) and one whose sub-channel has a reserved option (id 9)
        synth.fig0_2([{"sid": 0xC001, "components": [{"subchannel": 2, "ascty": 0}, {"subchannel": 3, "ascty": 0, "primary": False}]},
                      {"sid": 0xC002, "components": [{"subchannel": 20, "ascty": 63}, {"subchannel": 9, "ascty": 63}, {"subchannel": 1, "ascty": 63}]}]),
        # the next configuration and another ensemble's services do not count
        _fig0_2_raw(B((0xC003, 16), (0, 1), (0, 3), (1, 4)) + B((0, 2), (63, 6), (10, 6), (1, 1), (0, 1)), cn=1),
        _fig0_2_raw(B((0xC004, 16), (0, 1), (0, 3), (1, 4)) + B((0, 2), (63, 6), (10, 6), (1, 1), (0, 1)), oe=1),
    ]
    fibs = synth.pack_fibs(figs)
    assert len(fibs) <= 12
    filler = synth.pack_fibs([synth.fig0_0(0xC181, 0)])
    fib = np.concatenate([fibs] + [filler] * (12 - len(fibs)))[None]
    ok = np.ones((1, 12), np.uint8)
    got = comp_fields(dabgpu.fig_audio_components(fib, ok))
    assert got == [(0xC001, 2, 0, 0, 1), (0xE1C00123, 3, 100, 63, 0), (0xC002, 1, 300, 63, 1)] == walk_audio_components(fib, ok)
    # the sub-channels announced in the LAST FIB, behind the services that use them: the join does not depend on the order
    late = np.ascontiguousarray(fib[:, list(range(1, 12)) + [0]])
    assert comp_fields(dabgpu.fig_audio_components(late, ok)) == got == walk_audio_components(late, ok)
    # without FIG 0/1 nothing can be joined
    none = np.concatenate([synth.pack_fibs(figs[1:])] + [filler] * 12)[:12][None]
    assert dabgpu.fig_audio_components(none, ok) == []


def test_fig_audio_components_capacity(mixed):
    e = mixed[1]
    ok = np.ones((5, 12), np.uint8)
    L = dabgpu.lib()
    fib = np.ascontiguousarray(e.fibs)
    arr = (dabgpu.AudioComponent * 4)()
    for a in arr:
        a.subchid = -7
    n = C.c_int(-1)
    assert L.dabgpu_fig_audio_components(fib.ctypes.data, ok.ctypes.data, 5, arr, 3, C.byref(n)) == CAPACITY and n.value == 4
    assert all(a.subchid == -7 for a in arr)
    assert L.dabgpu_fig_audio_components(fib.ctypes.data, ok.ctypes.data, 5, None, 0, C.byref(n)) == CAPACITY and n.value == 4
    assert L.dabgpu_fig_audio_components(fib.ctypes.data, ok.ctypes.data, 5, arr, 4, C.byref(n)) == 0 and n.value == 4
    assert [a.subchid for a in arr] == [5, 4, 7, 9]
    with pytest.raises(dabgpu.DabGpuError) as err:
        dabgpu.fig_audio_components(e.fibs, ok, max_out=2)
    assert err.value.status == CAPACITY
    assert L.dabgpu_fig_audio_components(None, ok.ctypes.data, 5, arr, 4, C.byref(n)) == ARG
    assert L.dabgpu_fig_audio_components(fib.ctypes.data, ok.ctypes.data, 5, None, 4, C.byref(n)) == ARG


# ---- the reference's own properties
def test_erasure_frames_are_the_dispersal_sequence_and_no_raw_hit(built):
    assert F.dispersal_bytes(2).tolist() == [0x07, 0xBE]
    assert (np.packbits(synth.prbs(24 * 8 * 8)) == F.dispersal_bytes(24 * 8)).all()
    for s in (1, 8, 24, 64):
        assert not F.raw_hit(F.erasure_frames(1, s)[0])
    assert R.firecode(F.dispersal_bytes(11)[2:]) == 0xF097
    assert not F.raw_hit(np.zeros(24, np.uint8))                     # an all-zero header is its own check word


STREAM_SEEDS = {1: 301, 8: 308, 24: 324}


@pytest.mark.parametrize("s", [1, 8, 24])
def test_reference_emits_every_complete_superframe_whatever_the_chunking(built, s):
    for off in range(5):
        frames, sfs, starts = F.build_stream(STREAM_SEEDS[s] + 10 * off, 8 * s, 7, cut_frames=off, lead=2 if off == 3 else 0)
        first = 0 if off == 0 else 1
        want = sfs[first:, :110 * s]
        for size in (1, 4, 5, 7, 16, len(frames)):
            calls = F.follow_chunks(frames, s, F.cut(len(frames), size))
            data = np.concatenate([c[0] for c in calls])
            st = np.concatenate([c[1] for c in calls])
            assert (data == want).all() and st["firecode_ok"].all() and not st["rs_corrected"].any(), (off, size)
            assert sum(int(c[2]["dropped"]) for c in calls) == starts[0] and calls[-1][2]["held"] == 0, (off, size)
            assert calls[-1][2]["synced"] == 1


def test_new_kernels_neither_spill_nor_use_scratch(built, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the device assembly cannot be checked")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    out = tmp_path / "dabplus_kernels.s"
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "dabplus_kernels.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    md = kernel_metadata(out.read_text())
    one = lambda part: [v for k, v in md.items() if part in k]
    align, follow, aligned_sf = one("dabplus_align_kernel"), one("dabplus_follow_kernel"), one("dabplus_superframe_kernel")
    assert len(align) == len(follow) == len(aligned_sf) == 1
    for v in align + follow + aligned_sf:
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def fctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


IN_FILL, DATA_FILL, GAP = 0xC9, 0xA7, 64


def held_of(sp):
    """the frames the spec's carry record holds, as the call reads the record"""
    if sp.get("carry") is None:
        return 0
    held = int(np.asarray(sp["carry"][:16], np.uint8).view("<i4")[1])
    return held if 0 <= held <= 4 else 0


def decoy_count(sp, n_cifs):
    """the lanes of the last 64-frame block of the entry's held + n_cifs frames that have no frame"""
    return -(held_of(sp) + n_cifs) % 64


def call(ctx, specs, n_cifs, mutate=None, refused=False):
    """One follow call on device buffers laid out in one allocation, every region between sentinel bytes.
    specs: dicts {s, frames [n_cifs][24 s], carry (bytes of the record, or None = NULL), stride, shift (bytes the input is
    moved off its 256-byte boundary)}.  The whole allocation after the call must equal the allocation before it with the
    reference's outputs written in -- data rows and status records of the emitted super-frames only, the result record, the
    whole carry record -- or, for a call that must be refused (`mutate` spoils the table), the allocation before it.
    A spec's `decoy` (eleven bytes that pass F.raw_hit) is written where the frames behind the entry's last one would begin, at
    in + n_cifs stride, in + (n_cifs + 1) stride, ... for every lane the last 64-frame block of held + n_cifs frames leaves
    idle (decoy_count): inside the allocation, and nothing of the reference's outputs knows of them.
    -> per entry (data [n_sf][110 s], status [n_sf], result record, carry_out bytes) as the GPU wrote them."""
    import torch
    max_sf = (n_cifs + 4) // 5
    size, lay = 0, []

    def take(n, shift=0):
        nonlocal size
        off = (size + GAP + 255) // 256 * 256 + shift
        size = off + n
        return off

    for sp in specs:
        s = sp["s"]
        stride = sp.get("stride", 24 * s)
        n_decoys = decoy_count(sp, n_cifs) if sp.get("decoy") is not None else 0
        lay.append({"in": take(max(n_cifs + n_decoys - 1, 0) * stride + 24 * s, sp.get("shift", 0)),
                    "cin": take(F.carry_bytes(s)) if sp.get("carry") is not None else None, "cout": take(F.carry_bytes(s)),
                    "data": take(max_sf * 110 * s, sp.get("shift", 0)), "status": take(max_sf * 64), "result": take(32)})
    before = np.full(size + GAP, DATA_FILL, np.uint8)
    rng = np.random.default_rng(size)
    for sp, L in zip(specs, lay):
        s = sp["s"]
        stride = sp.get("stride", 24 * s)
        frames = np.asarray(sp["frames"], np.uint8).reshape(n_cifs, 24 * s)
        before[L["in"]:L["in"] + max(n_cifs - 1, 0) * stride + 24 * s] = rng.integers(0, 256, max(n_cifs - 1, 0) * stride + 24 * s, dtype=np.uint8)
        for i in range(n_cifs):
            before[L["in"] + i * stride:L["in"] + i * stride + 24 * s] = frames[i]
        if sp.get("decoy") is not None:
            decoy = np.asarray(sp["decoy"], np.uint8)
            assert decoy.shape == (11,) and F.raw_hit(decoy)
            for i in range(n_cifs, n_cifs + decoy_count(sp, n_cifs)):
                before[L["in"] + i * stride:L["in"] + i * stride + 24 * s] = rng.integers(0, 256, 24 * s, dtype=np.uint8)
                before[L["in"] + i * stride:L["in"] + i * stride + 11] = decoy
        if L["cin"] is not None:
            before[L["cin"]:L["cin"] + F.carry_bytes(s)] = sp["carry"]
    t = torch.from_numpy(before).cuda()
    base = t.data_ptr()
    assert base % 256 == 0
    entries = [dabgpu.DabplusEntry(base + L["in"], sp.get("stride", 24 * sp["s"]), 8 * sp["s"], base + L["cin"] if L["cin"] is not None else None,
                                   base + L["cout"], base + L["data"], base + L["status"], base + L["result"])
               for sp, L in zip(specs, lay)]
    if mutate:
        mutate(entries)
    if refused:
        with pytest.raises(dabgpu.DabGpuError) as err:
            ctx.dabplus_follow_dev(entries, n_cifs)
        assert err.value.status == ARG
        ctx.sync()
        assert (t.cpu().numpy() == before).all(), "a refused call wrote"
        return None
    ctx.dabplus_follow_dev(entries, n_cifs)
    ctx.sync()
    after = t.cpu().numpy()
    want = before.copy()
    out = []
    for sp, L in zip(specs, lay):
        s = sp["s"]
        data, st, res, cout = F.follow(sp["frames"], s, sp.get("carry"))
        n = len(data)
        want[L["data"]:L["data"] + n * 110 * s] = data.reshape(-1)
        want[L["status"]:L["status"] + n * 64] = st.view(np.uint8).reshape(-1)
        want[L["result"]:L["result"] + 32] = np.frombuffer(res.tobytes(), np.uint8)
        want[L["cout"]:L["cout"] + F.carry_bytes(s)] = cout
        g_res = after[L["result"]:L["result"] + 32].copy().view(F.RESULT_DTYPE)[0]
        g_n = max(0, min(int(g_res["n_superframes"]), max_sf))
        out.append((after[L["data"]:L["data"] + g_n * 110 * s].reshape(g_n, 110 * s).copy(),
                    after[L["status"]:L["status"] + g_n * 64].copy().view(dabgpu.SUPERFRAME_STATUS_DTYPE), g_res,
                    after[L["cout"]:L["cout"] + F.carry_bytes(s)].copy()))
    bad = np.flatnonzero(after != want)
    if bad.size:
        at = int(bad[0])
        where = [(e, k) for e, L in enumerate(lay) for k, v in L.items() if v is not None and v <= at]
        e, k = max(where, key=lambda w: lay[w[0]][w[1]]) if where else (-1, "?")
        raise AssertionError("%d bytes differ from the reference; the first at %d: entry %d, %d bytes into (or behind) its '%s'; "
                             "result %s, reference %s" % (bad.size, at, e, at - lay[e][k] if e >= 0 else 0, k, out[e][2] if e >= 0 else None,
                                                          F.follow(specs[e]["frames"], specs[e]["s"], specs[e].get("carry"))[2] if e >= 0 else None))
    return out


def run_chunks(ctx, frames, s, chunks, carry=None, **kw):
    """one entry fed in calls of `chunks` frames, each call's carry record handed to the next -> the calls' results"""
    got, at = [], 0
    for n in chunks:
        r = call(ctx, [dict(s=s, frames=frames[at:at + n], carry=carry, **kw)], n)[0]
        got.append(r)
        carry = r[3]
        at += n
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1, 8, 24])
def test_gpu_alignment_and_chunking(fctx, s):
    """a 7-super-frame stream at the five offsets, in calls of 1, 4, 5, 7 and 16 CIFs and in one: every call equals the
    reference (inside call()), the concatenated output equals the single call's and the transmitted super-frames"""
    for off in range(5):
        frames, sfs, starts = F.build_stream(STREAM_SEEDS[s] + 10 * off, 8 * s, 7, cut_frames=off, lead=2 if off == 3 else 0)
        single = call(fctx, [dict(s=s, frames=frames)], len(frames))[0]
        assert single[2]["phase"] == starts[0] % 5 and single[2]["n_superframes"] == len(starts) == len(single[0])
        assert (single[0] == sfs[7 - len(starts):, :110 * s]).all() and single[1]["firecode_ok"].all()
        for size in (1, 4, 5, 7, 16):
            calls = run_chunks(fctx, frames, s, F.cut(len(frames), size), shift=size % 3, stride=24 * s + (size & 4))
            assert (np.concatenate([c[0] for c in calls]) == single[0]).all(), (off, size)
            assert (np.concatenate([c[1] for c in calls]).view(np.uint8) == single[1].view(np.uint8)).all(), (off, size)
            assert calls[-1][2]["held"] == 0 and calls[-1][2]["synced"] == 1


def damage_columns(sf, s, rng, n_errors):
    """n_errors byte errors in every column of one super-frame, none in the first 11 bytes of a logical frame (the raw
    headers -- hits and misses -- stay what they were)"""
    for j in range(s):
        rows = [i for i in range(120) if (j + s * i) % (24 * s) >= 11]
        for i in rng.choice(rows, n_errors, replace=False):
            sf[j + s * i] ^= rng.integers(1, 256, dtype=np.uint8)


RAGGED_BITRATES = [8, 32, 48, 64, 128, 192, 192, 128, 64, 48, 32, 8, 64]


@pytest.fixture(scope="module")
def ragged(fctx):
    """13 entries in one call, twice: 7 CIFs, then 13 with the first call's carry for some entries and a fresh start (NULL)
    for the others.  Own bit rate, offset, in_stride (tight and padded), input address (aligned and not); entry 12 is all
    erasures.  -> (specs of the second call, its results)"""
    rng = np.random.default_rng(77)
    streams = []
    for e, br in enumerate(RAGGED_BITRATES):
        s = br // 8
        if e == 12:
            streams.append(F.erasure_frames(20, s))
            continue
        frames, sfs, starts = F.build_stream(500 + e, br, 5, cut_frames=e % 5, lead=(e // 5) % 3, combo=[(1, 0), (0, 1), (1, 1), (0, 0)][e % 4])
        frames = frames[:20].copy()
        for k in range(0, 16, 5):                                 # byte errors in the super-frames the 20 frames hold whole
            a = starts[0] + k
            if e % 2 and a + 5 <= 20:
                sf = frames[a:a + 5].reshape(-1)
                damage_columns(sf, s, rng, 1 + (e + k) % 5)
                frames[a:a + 5] = sf.reshape(5, 24 * s)
        streams.append(frames)
    geometry = [dict(stride=24 * (br // 8) + [0, 5, 16, 0, 40][e % 5], shift=[0, 1, 16, 3, 8, 0][e % 6]) for e, br in enumerate(RAGGED_BITRATES)]
    first = call(fctx, [dict(s=br // 8, frames=streams[e][:7], **geometry[e]) for e, br in enumerate(RAGGED_BITRATES)], 7)
    specs = []
    for e, br in enumerate(RAGGED_BITRATES):
        fresh = e % 3 == 2
        specs.append(dict(s=br // 8, frames=streams[e][7:], carry=None if fresh else first[e][3], **geometry[e]))
    return specs, call(fctx, specs, 13)


@pytest.mark.gpu
def test_gpu_ragged_batch_in_one_call(ragged):
    specs, got = ragged                                           # (byte for byte against the reference, sentinels included: call())
    assert len(specs) >= 12 and {8 * sp["s"] for sp in specs} == {8, 32, 48, 64, 128, 192}
    assert any(sp["carry"] is None for sp in specs[:12]) and any(sp["carry"] is not None for sp in specs[:12])
    assert {sp["shift"] % 16 == 0 for sp in specs} == {True, False} and {sp["stride"] == 24 * sp["s"] for sp in specs} == {True, False}
    assert got[12][2]["phase"] == -1 and got[12][2]["n_superframes"] == 0 and got[12][2]["raw_hits"] == 0
    assert all(r[2]["n_superframes"] >= 1 and r[2]["synced"] == 1 for r in got[:12])
    assert len({int(r[2]["phase"]) for r in got[:12]}) >= 3
    assert sum(int(r[1]["rs_corrected"].sum()) for r in got[:12]) > 100 and all(r[1]["firecode_ok"].all() for r in got[:12])


@pytest.mark.gpu
def test_gpu_emitted_superframes_equal_the_existing_call(fctx, ragged):
    from test_dabplus_superframes import run_dev
    specs, got = ragged
    n = 0
    for sp, (data, st, res, _c) in zip(specs, got):
        s = sp["s"]
        held = int(np.asarray(sp["carry"][:16]).view("<i4")[1]) if sp["carry"] is not None else 0
        seq = np.concatenate([np.asarray(sp["carry"][16:16 + held * 24 * s]).reshape(held, 24 * s), sp["frames"]]) if held else sp["frames"]
        p = int(res["phase"])
        for k in range(int(res["n_superframes"])):
            out, st1 = run_dev(fctx, seq[p + 5 * k:p + 5 * k + 5].reshape(1, 120 * s), s)
            assert (out[0] == data[k]).all() and st1.tobytes() == st[k:k + 1].tobytes(), (s, k)
            n += 1
    assert n >= 12


def _header_errors(frames, start, s, rng):
    """every one of the 11 header bytes of the super-frame starting at frame `start` wrong: at most 2 errors a column
    (s = 8), which RS repairs -- and the raw check misses"""
    frames[start, :11] ^= rng.integers(1, 256, 11, dtype=np.uint8)
    assert not F.raw_hit(frames[start])


@pytest.mark.gpu
def test_gpu_errors_votes_and_lost_frames(fctx):
    s, rng = 8, np.random.default_rng(91)
    # a header with byte errors: raw miss, emitted where the others' votes put it, firecode_ok after RS
    frames, sfs, starts = F.build_stream(611, 64, 5, cut_frames=3)
    _header_errors(frames, starts[1], s, rng)
    data, st, res, _c = call(fctx, [dict(s=s, frames=frames)], len(frames))[0]
    assert (res["phase"], res["n_superframes"], res["raw_hits"], res["synced"]) == (2, 4, 3, 1)
    assert st["firecode_ok"].tolist() == [1, 1, 1, 1] and st["rs_corrected"].tolist() == [0, 11, 0, 0] and (data == sfs[1:, :880]).all()
    # one super-frame beyond repair: emitted with firecode_ok = 0, sync kept, the next ones come out
    frames, sfs, starts = F.build_stream(612, 64, 4, cut_frames=0, lead=1)
    frames[starts[1]:starts[1] + 5] = rng.integers(0, 256, (5, 192), dtype=np.uint8)
    assert not any(F.raw_hit(f) for f in frames[starts[1]:starts[1] + 5])
    calls = run_chunks(fctx, frames, s, [11, 10])
    st = np.concatenate([c[1] for c in calls])
    assert st["firecode_ok"].tolist() == [1, 0, 1, 1] and st["rs_uncorrectable"][1] > 0
    assert [int(c[2]["synced"]) for c in calls] == [1, 1] and calls[1][2]["phase"] == 0 and calls[1][2]["dropped"] == 0
    # a synced call in which no start frame hits raw: the phase is kept, the super-frames come out, synced_out = 0
    frames, sfs, starts = F.build_stream(613, 64, 4)
    _header_errors(frames, 10, s, rng)
    _header_errors(frames, 15, s, rng)
    calls = run_chunks(fctx, frames, s, [10, 10])
    assert calls[1][2]["raw_hits"] == 0 and calls[1][2]["phase"] == 0 and calls[1][2]["n_superframes"] == 2 and calls[1][2]["synced"] == 0
    assert calls[1][1]["firecode_ok"].tolist() == [1, 1] and (calls[1][0] == sfs[2:, :880]).all()
    # ... and the same call on a fresh start finds nothing: that is what the carry is for
    lost = call(fctx, [dict(s=s, frames=frames[10:])], 10)[0]
    assert lost[2]["phase"] == -1 and lost[2]["n_superframes"] == 0 and lost[2]["held"] == 4 and lost[2]["dropped"] == 6
    # one logical frame lost between two calls: the next call's votes move the phase, `dropped` says so
    frames, sfs, starts = F.build_stream(614, 64, 5)
    a = call(fctx, [dict(s=s, frames=frames[:10])], 10)[0]
    b = call(fctx, [dict(s=s, frames=frames[11:], carry=a[3])], 14)[0]
    assert (a[2]["synced"], a[2]["held"]) == (1, 0)
    assert (b[2]["phase"], b[2]["dropped"], b[2]["n_superframes"], b[2]["synced"]) == (4, 4, 2, 1) and (b[0] == sfs[3:, :880]).all()
    # a synced carry, one vote for residue 0 and one for residue 2: the phase stays 0; two votes for residue 2 move it
    one, _sfs, _st = F.build_stream(615, 64, 1)
    two, _sfs, _st = F.build_stream(616, 64, 2)
    synced = np.zeros(F.carry_bytes(s), np.uint8)
    synced[:4].view("<i4")[0] = 1
    tie = np.concatenate([one, F.erasure_frames(2, s), two[:3]])
    r = call(fctx, [dict(s=s, frames=tie, carry=synced)], 10)[0]
    assert (r[2]["raw_hits"], r[2]["phase"], r[2]["n_superframes"], r[2]["dropped"]) == (2, 0, 2, 0) and r[1]["firecode_ok"].tolist() == [1, 0]
    more = np.concatenate([one, F.erasure_frames(2, s), two])
    r = call(fctx, [dict(s=s, frames=more, carry=synced)], 17)[0]
    assert (r[2]["raw_hits"], r[2]["phase"], r[2]["n_superframes"], r[2]["dropped"]) == (3, 2, 3, 2) and r[1]["firecode_ok"].tolist() == [0, 1, 1]
    # an all-zero carry record is a fresh start: the same as NULL
    z = call(fctx, [dict(s=s, frames=tie, carry=np.zeros(F.carry_bytes(s), np.uint8))], 10)[0]
    n = call(fctx, [dict(s=s, frames=tie)], 10)[0]
    assert z[2].tobytes() == n[2].tobytes() and z[3].tobytes() == n[3].tobytes()


@pytest.mark.gpu
def test_gpu_refused_calls_leave_every_output_alone(fctx):
    """a bad entry LATE in the table: nothing of the good entries before it is written (sentinels: call())"""
    frames, _sfs, _st = F.build_stream(620, 64, 2)
    carry = F.follow(frames[:3], 8)[3]
    specs = [dict(s=8, frames=frames[3:], carry=carry) for _ in range(4)]

    def spoil(field, value):
        def f(entries):
            setattr(entries[3], field, value(entries[3]) if callable(value) else value)
        return f

    for m in (spoil("bitrate_kbps", 12), spoil("bitrate_kbps", 0), spoil("bitrate_kbps", 520), spoil("in_stride", 191),
              spoil("d_carry_out", lambda e: e.d_carry_in), spoil("d_carry_out", lambda e: e.d_carry_in + 16),
              spoil("d_carry_out", None), spoil("d_carry_in", lambda e: e.d_carry_in + 4), spoil("d_result", None),
              spoil("d_in", None), spoil("d_data", None), spoil("d_status", lambda e: e.d_status + 2)):
        call(fctx, specs, 7, mutate=m, refused=True)
    with pytest.raises(dabgpu.DabGpuError):
        fctx.dabplus_follow_dev([dabgpu.DabplusEntry()], -1)
    fctx.dabplus_follow_dev([], 16)                                # nothing to do is not an error
    got = call(fctx, specs, 7)                                     # ... and the unspoilt table goes through
    assert all(r[2]["n_superframes"] == 2 for r in got)


# ---- end to end
E2E_SERVICES = [("Radio One", 0xC221, 3, 0, 3, 64, 0), ("Jazz 24", 0xC222, 7, 0, 2, 48, 48), ("News", 0xC223, 9, 1, 2, 32, 200)]   # test_fig.py
E2E_DAB = [("Classic", 0xC332, 11, 17, 100)]                                                                       # test_fig.py


@pytest.mark.gpu
def test_gpu_end_to_end_iq_to_access_units(fctx):
    """IQ of one self-describing multiplex received from transmission frame 0 and from frame 1 (super-frame phases 0 and 1 in
    the decoder's output) -> front end -> FIC pass -> fig_subchannels + fig_audio_components -> decode_ensembles_dev ->
    follow, in two consecutive calls of 16 frames: the access units of every DAB+ service, in order, across the boundary"""
    import torch
    dev = torch.device("cuda", 0)
    fps, n_calls, L = 16, 2, 76 * 2552
    ens = synth.ServiceEnsemble(3, E2E_SERVICES, n_frames=5, dab_services=E2E_DAB, extras=False)
    tx = ens.iq()
    rng = np.random.default_rng(12)
    c = fctx
    c.streams_reset(2)
    plans = comps = None
    followed = hist = carry = None
    got = [[[] for _ in E2E_SERVICES] for _ in range(2)]             # [stream][service] -> (start frame t, AU index, bytes)
    whole = [[[] for _ in E2E_SERVICES] for _ in range(2)]           # ... -> start frames of super-frames with every AU clean
    held_in = [[0] * 3 for _ in range(2)]
    phases = []
    for call_no in range(n_calls):
        iq = []
        for k in range(2):
            idx = (np.arange(fps) + call_no * fps + k) % 5
            rx = synth.channel(tx[idx].ravel(), snr_db=20.0, rng=rng).reshape(fps, -1)
            iq.append(rx[:, synth.NB_NULL:synth.NB_NULL + L])
        d_iq = torch.from_numpy(np.concatenate(iq).astype(np.complex64)).to(dev)
        d_soft = torch.zeros((2 * fps, FB), dtype=torch.int8, device=dev)
        c.ofdm_demod_streams_dev(d_iq.data_ptr(), L, 2, fps, 0.9, d_soft.data_ptr(), None, None)
        fib = torch.zeros((2 * fps, 12, 32), dtype=torch.uint8, device=dev)
        ok = torch.zeros((2 * fps, 12), dtype=torch.uint8, device=dev)
        if plans is None:
            c.decode_ensembles_dev(d_soft.data_ptr(), FB, 2, fps, fib.data_ptr(), ok.data_ptr(), [[], []], None, None, None, None)
            c.sync()
            fib_h, ok_h = fib.cpu().numpy(), ok.cpu().numpy()
            assert ok_h.all()
            plans = [dabgpu.fig_subchannels(fib_h[k * fps:(k + 1) * fps], ok_h[k * fps:(k + 1) * fps]) for k in range(2)]
            comps = [dabgpu.fig_audio_components(fib_h[k * fps:(k + 1) * fps], ok_h[k * fps:(k + 1) * fps]) for k in range(2)]
            for k in range(2):
                assert [sc.start_address for sc in plans[k]] == [cp.start_address for cp in comps[k]] == [0, 48, 100, 200]
                assert [cp.ascty for cp in comps[k]] == [63, 63, 0, 63] and comps[k][2].subchid == 11
            # the DAB service's entry is decoded but not followed
            followed = [[j for j, cp in enumerate(comps[k]) if cp.ascty == dabgpu.ASCTY_DABPLUS] for k in range(2)]
            assert followed == [[0, 1, 3], [0, 1, 3]]
            hist = [[[torch.zeros((15, sc.length * 64), dtype=torch.int8, device=dev) for sc in p] for p in plans] for _ in range(2)]
            carry = [[[torch.zeros(dabgpu.dabplus_carry_bytes(plans[k][j].bitrate_kbps), dtype=torch.uint8, device=dev) for j in followed[k]]
                      for k in range(2)] for _ in range(2)]
        outs = [[torch.zeros((fps * 4, sc.bitrate_kbps * 3), dtype=torch.uint8, device=dev) for sc in p] for p in plans]
        ptrs = lambda lsts: [[x.data_ptr() for x in lst] for lst in lsts]
        c.decode_ensembles_dev(d_soft.data_ptr(), FB, 2, fps, fib.data_ptr(), ok.data_ptr(), plans, ptrs(hist[0]) if call_no else None,
                               ptrs(hist[1]), ptrs(outs), None)
        n_cifs, max_sf = 4 * fps, (4 * fps + 4) // 5
        entries, bufs = [], []
        for k in range(2):
            for n, j in enumerate(followed[k]):
                br = plans[k][j].bitrate_kbps
                data = torch.zeros((max_sf, 110 * br // 8), dtype=torch.uint8, device=dev)
                st = torch.zeros((max_sf * 64,), dtype=torch.uint8, device=dev)
                res = torch.zeros((32,), dtype=torch.uint8, device=dev)
                bufs.append((k, n, data, st, res))
                # the first call starts fresh (an all-zero record would do as well); then the records swap
                entries.append(dabgpu.DabplusEntry(outs[k][j].data_ptr(), 3 * br, br, carry[0][k][n].data_ptr() if call_no else None,
                                                   carry[1][k][n].data_ptr(), data.data_ptr(), st.data_ptr(), res.data_ptr()))
        c.dabplus_follow_dev(entries, n_cifs)
        c.sync()
        hist.reverse()
        carry.reverse()
        for k, n, data, st, res in bufs:
            r = res.cpu().numpy().view(dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)[0]
            stat = st.cpu().numpy().view(dabgpu.SUPERFRAME_STATUS_DTYPE)[:r["n_superframes"]]
            d = data.cpu().numpy()
            phases.append((call_no, k, int(r["phase"]), int(r["synced"])))
            for q in range(int(r["n_superframes"])):
                t = call_no * n_cifs - held_in[k][n] + int(r["phase"]) + 5 * q    # the decoder output the super-frame starts at
                if not stat[q]["firecode_ok"]:
                    continue
                clean = [a for a in range(int(stat[q]["num_aus"])) if stat[q]["au_crc_mask"] >> a & 1]
                got[k][n] += [(t, a, d[q, stat[q]["au_start"][a]:stat[q]["au_start"][a + 1]]) for a in clean]
                if len(clean) == 3:
                    whole[k][n].append(t)
            held_in[k][n] = int(r["held"])
    # decoder output t of stream k is logical frame (t - 15 + 4 k) of the cyclic multiplex: the first super-frame starts at
    # t = 15 (phase 0) and t = 16 (phase 1); after 64 CIFs 4 and 3 frames are carried, and the second call stays on phase 0
    assert sorted(phases) == sorted([(0, 0, 0, 1)] * 3 + [(0, 1, 1, 1)] * 3 + [(1, 0, 0, 1)] * 3 + [(1, 1, 0, 1)] * 3)
    # Every CRC-clean access unit is the transmitted one, in order; from t0 on (the de-interleaver has all sixteen CIFs of a
    # logical frame) every super-frame is there whole.  (Before t0 a frame is decoded from part of its bits: what comes out
    # clean is right as well, and how much does is the channel decoder's business.)
    for k in range(2):
        t0 = 15 + k
        for n in range(3):
            assert whole[k][n][-len(range(t0, 4 * fps * n_calls - 4, 5)):] == list(range(t0, 4 * fps * n_calls - 4, 5)), (k, n, whole[k][n])
            assert [t for t, _a, _b in got[k][n]] == sorted(t for t, _a, _b in got[k][n]) and len(got[k][n]) >= 3 * 22
            for t, a, au in got[k][n]:
                assert (t - t0) % 5 == 0
                w = ens.aus[n][((t - 15 + 4 * k) // 5) % 4][a]
                assert au.size == w.size and (au == w).all(), (k, n, t, a)
