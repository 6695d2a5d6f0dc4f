"""ETI(NI) input (include/dabgpu.h, "ETI(NI) input"): byte streams read back into FIBs, CRC flags and logical frames.
The host twin is held byte for byte to tests/eti_read_reference.py (the contract in plain Python), the device call byte for
byte to the host twin -- rows, status, result and state; outputs start out as 0xEE so that what a call must not write is
compared too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dabgpu
import eti_read_reference as RR
import eti_reference as R
from conftest import ROOT, make_ctx
from dabgpu import synth
from test_eti import CONFIGS, ref_stream

FRAME = 6144
STATE_BYTES = 80 + 6144
FILL = 0xEE


# ------------------------------------------------------------------ streams and damage
def make_fibs(rng, n_cif, bad_every=7):
    """[n_cif][3][32] random FIBs, the CRC right on all but every bad_every-th FIB, and the flags that go with them."""
    fibs = rng.integers(0, 256, (n_cif, 3, 32), dtype=np.uint8)
    ok = np.ones((n_cif, 3), np.uint8)
    for c in range(n_cif):
        for j in range(3):
            crc = synth.crc16(fibs[c, j, :30].tobytes())
            fibs[c, j, 30], fibs[c, j, 31] = crc >> 8, crc & 0xFF
            if (3 * c + j) % bad_every == bad_every - 1:
                fibs[c, j, 5] ^= 0x40
                ok[c, j] = 0
    return fibs, ok


def make_frames(name, n_cif, seed, start=0):
    """n_cif frames of configuration `name` from the reference writer -> (list of 6144-byte frames, stream dicts)."""
    rng = np.random.default_rng(seed)
    ref = [ref_stream(i, sc) for i, sc in CONFIGS[name]()]
    fibs, ok = make_fibs(rng, n_cif)
    data = {st["id"]: rng.integers(0, 256, (n_cif, st["bitrate"] * 3), dtype=np.uint8) for st in ref}
    hist = {"fibs": [fibs[0]] * 15, "crc_ok": [ok[0]] * 15, "next_count": start} if seed % 2 else None   # odd seeds: no warm-up
    frames, _, _ = R.write_stream(ref, fibs, ok, data, history=hist, cif_start=start)
    return frames, ref


def flip(frame, pos, bit=0):
    b = bytearray(frame)
    b[pos] ^= 1 << bit
    return bytes(b)


def chunk_flips(frame, ref):
    """64 copies of the frame, copy i with a bit flipped in chunk i of the 64 the data CRC is folded in (zero words in front
    up to 64 equal chunks; a chunk that is all padding gives a flip in the first data byte instead)."""
    nst = len(ref)
    fic0, n_words = 12 + 4 * nst, (96 + sum(st["bitrate"] * 3 for st in ref)) // 4
    cw = (n_words + 63) // 64
    lead = 64 * cw - n_words
    out = []
    for i in range(64):
        m = max(i * cw - lead + (cw - 1), 0)
        out.append(flip(frame, fic0 + 4 * m + i % 4, i % 8))
    return out


def damage_set(name, seed):
    """A stream of configuration `name` with every kind of damage, as one byte string, and its plan."""
    frames, ref = make_frames(name, 40, seed, start=245)
    nst = len(ref)
    hdr_last, fic0 = 11 + 4 * nst, 12 + 4 * nst
    eof = R.frame_length(ref)[1] - 8
    f = list(frames)
    f[2] = flip(f[2], 4, 1)                                   # the header span's first byte (FCT)
    f[4] = flip(f[4], hdr_last, 7)                            # ... and its last (the CRC's low byte)
    f[6] = flip(f[6], fic0, 0)                                # the data span's first byte
    f[8] = flip(f[8], eof + 1, 3)                             # ... and its last (the CRC's low byte)
    b = bytearray(f[10])                                      # the sync of the other parity
    b[1:4] = R.FSYNC_EVEN if b[4] & 1 else R.FSYNC_ODD
    f[10] = bytes(b)
    other, _ = make_frames("tiny" if name != "tiny" else "one_eep_a", 1, seed + 2, start=245 + 12)
    f[12] = other[0]                                          # a frame of another multiplex
    f[14] = f[14][:100] + f[14][101:]                         # 1 byte gone
    f[16] = f[16][:3000] + f[16][3017:]                       # 17 bytes gone
    f[18] = f[18][:1]                                         # 6143 bytes gone
    f[20] = f[20][:50] + b"\x01\x02\x03\x04\x05" + f[20][50:]  # 5 bytes too many
    del f[23:26]                                              # an FCT jump
    if eof - fic0 - 96 >= 300:                                # a sync pattern, a whole header, planted inside the data:
        g = bytearray(f[28])                                  # (the frame's own data CRC is made right again, so only the
        g[fic0 + 96:fic0 + 96 + 12 + 4 * nst] = f[29][:12 + 4 * nst]   # walk's step of 6144 keeps it from being taken for a frame)
        crc = synth.crc16(bytes(g[fic0:eof]))
        g[eof:eof + 2] = bytes([crc >> 8, crc & 0xFF])
        f[28] = bytes(g)
    f[-1] = f[-1][:1234]                                      # the stream ends inside a frame
    return b"".join(f), ref


# ------------------------------------------------------------------ running the calls
def aligned(n, fill=FILL):
    raw = np.full(n + 16, fill, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n]


class Case:
    """One entry: plan streams [(scid, Subchannel)] or None, the new bytes, the state record (uint8 [STATE_BYTES]) or None,
    which streams are wanted (None: all)."""

    def __init__(self, streams, data, state=None, wanted=None):
        self.streams, self.data, self.state, self.wanted = streams, bytes(data), state, wanted
        self.plan = None if streams is None else dabgpu.eti_layout(streams)
        self.rows = dabgpu.eti_read_max_frames(len(self.data))
        self.sizes = [] if streams is None else [sc.bitrate_kbps * 3 for _, sc in streams]
        if wanted is None:
            self.wanted = [True] * len(self.sizes)


def _entry(case, addr, keep):
    """addr(array) -> address; arrays: dict of the case's buffers"""
    a = case.arrays
    ptrs = (C.c_void_p * max(len(case.sizes), 1))(*[addr(o) if w else 0 for o, w in zip(a["outs"], case.wanted)])
    keep.append(ptrs)
    return dabgpu.EtiReadEntry(addr(a["bytes"]) if len(case.data) else None, len(case.data), 0,
                               C.pointer(case.plan) if case.plan is not None else None,
                               C.cast(ptrs, C.POINTER(C.c_void_p)) if case.plan is not None else None,
                               None if a["state_in"] is None else addr(a["state_in"]), addr(a["state_out"]), addr(a["fib"]),
                               addr(a["crc_ok"]), addr(a["status"]), addr(a["result"]))


def _collect(case, get):
    a = case.arrays
    return {"fib": get(a["fib"]).reshape(-1, 96), "crc_ok": get(a["crc_ok"]).reshape(-1, 3),
            "outs": [get(o).reshape(max(case.rows, 1), -1) for o in a["outs"]],
            "status": get(a["status"]).view(dabgpu.ETI_READ_STATUS_DTYPE).reshape(-1),
            "result": get(a["result"]).view(dabgpu.ETI_READ_RESULT_DTYPE)[0], "state": get(a["state_out"])}


def run_host(cases):
    keep, entries = [], []
    for c in cases:
        c.arrays = {"bytes": aligned(max(len(c.data), 1)), "state_in": None, "state_out": aligned(STATE_BYTES),
                    "fib": aligned(max(c.rows, 1) * 96), "crc_ok": aligned(max(c.rows, 1) * 3), "status": aligned(max(c.rows, 1) * 16),
                    "result": aligned(48), "outs": [aligned(max(c.rows, 1) * n) for n in c.sizes]}
        c.arrays["bytes"][:len(c.data)] = np.frombuffer(c.data, np.uint8)
        if c.state is not None:
            c.arrays["state_in"] = aligned(STATE_BYTES)
            c.arrays["state_in"][:] = c.state
        entries.append(_entry(c, lambda x: x.ctypes.data, keep))
    dabgpu.eti_read_host(entries)
    return [_collect(c, lambda x: x.copy()) for c in cases]


def run_dev(ctx, cases):
    import torch
    keep, entries = [], []
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    full = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    for c in cases:
        rows = max(c.rows, 1)
        c.arrays = {"bytes": dev(np.frombuffer(c.data or b"\0", np.uint8).copy()), "state_in": None if c.state is None else dev(c.state),
                    "state_out": full(STATE_BYTES), "fib": full(rows * 96), "crc_ok": full(rows * 3), "status": full(rows * 16),
                    "result": full(48), "outs": [full(rows * n) for n in c.sizes]}
        entries.append(_entry(c, lambda x: x.data_ptr(), keep))
    ctx.eti_read_dev(entries)
    ctx.sync()
    return [_collect(c, lambda x: x.cpu().numpy()) for c in cases]


def assert_same(a, b, what=""):
    """two results of _collect, byte for byte"""
    for k in ("result", "status", "fib", "crc_ok", "state"):
        x, y = np.atleast_1d(a[k]).view(np.uint8).reshape(-1), np.atleast_1d(b[k]).view(np.uint8).reshape(-1)
        if x.tobytes() != y.tobytes():
            bad = np.nonzero(x != y)[0]
            pytest.fail("%s %s differs at bytes %s (%d in all): %s / %s" % (what, k, bad[:8], bad.size, a["result"], b["result"]))
    for i, (x, y) in enumerate(zip(a["outs"], b["outs"])):
        assert x.tobytes() == y.tobytes(), "%s stream %d differs" % (what, i)


def state_of_record(rec):
    """a record the library wrote -> the reference's state"""
    h = rec[:80].view(dabgpu.ETI_READ_HEAD_DTYPE)[0]
    n = min(int(h["tail_bytes"]), 6143)
    return {"tail": rec[80:80 + n].tobytes(), "have_prev": bool(h["have_prev"]), "last_fct": int(h["last_fct"]),
            "last_fp": int(h["last_fp"]), "totals": {k: int(h[k]) for k in RR.COUNTERS}}


def assert_is_reference(case, got, state=None, what=""):
    """the host twin's (or the device's) outputs of one case against the reference reader"""
    plan = None if case.streams is None else [ref_stream(i, sc) for i, sc in case.streams]
    rows, result, new = RR.read(state, case.data, plan)
    res = got["result"]
    assert {k: int(res[k]) for k in RR.COUNTERS + ("tail_bytes",)} == result, (what, res, result)
    assert not res["reserved"].any()
    n = len(rows)
    for r, row in enumerate(rows):
        st = got["status"][r]
        assert tuple(int(st[k]) for k in ("offset", "verdict", "fct", "fp", "err", "fib_ok", "gap", "flags", "reserved", "reserved2")) == \
            (row["offset"], row["verdict"], row["fct"], row["fp"], row["err"], row["fib_ok"], row["gap"], row["flags"], 0, 0), (what, r, st, row)
        assert got["fib"][r].tobytes() == row["fic"] and list(got["crc_ok"][r]) == row["crc_ok"], (what, r)
        for k, (scid, _) in enumerate(case.streams or []):
            if case.wanted[k]:
                assert got["outs"][k][r].tobytes() == row["data"][scid], (what, r, k)
    # nothing behind the emitted rows, and nothing for a stream that is not wanted
    assert (got["fib"][n:] == FILL).all() and (got["crc_ok"][n:] == FILL).all() and (got["status"].view(np.uint8)[16 * n:] == FILL).all()
    for k, o in enumerate(got["outs"]):
        assert (o[n if case.wanted[k] else 0:] == FILL).all()
    head = got["state"][:80].view(dabgpu.ETI_READ_HEAD_DTYPE)[0]
    assert state_of_record(got["state"]) == new, what
    assert int(head["tail_bytes"]) == len(new["tail"]) and not got["state"][80 + len(new["tail"]):].any()
    assert int(head["reserved"]) == 0 and int(head["reserved2"]) == 0
    return rows, result, new


# ------------------------------------------------------------------ CPU
def test_struct_layouts_match_the_header(tmp_path):
    records = [("dabgpu_eti_read_status", dabgpu.ETI_READ_STATUS_DTYPE), ("dabgpu_eti_read_result", dabgpu.ETI_READ_RESULT_DTYPE)]
    cls = dabgpu.EtiReadEntry
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dabgpu.h"', 'int main(void) {']
    for cname, fields in [("dabgpu_eti_read_entry", [f for f, _ in cls._fields_])] + [(c, list(dt.names)) for c, dt in records]:
        lines.append('  printf("%s %%zu", sizeof(%s));' % (cname, cname))
        lines += ['  printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f in fields]
        lines.append('  printf("\\n");')
    lines.append('  printf("%d %d %d %d %d %d\\n", DABGPU_ETI_BAD_DATA_CRC, DABGPU_ETI_OTHER_PLAN, DABGPU_ETI_READ_GAP, '
                 'DABGPU_ETI_READ_FP_BREAK, DABGPU_ETI_READ_ERR_FIELD, DABGPU_ETI_READ_FIB_CRC);')
    lines += ['  return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(x) for x in out[0].split()[1:]] == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    for (cname, dt), line in zip(records, out[1:]):
        assert line.split()[0] == cname and [int(x) for x in line.split()[1:]] == [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    assert [int(x) for x in out[3].split()] == [dabgpu.ETI_BAD_DATA_CRC, dabgpu.ETI_OTHER_PLAN, dabgpu.ETI_READ_GAP, dabgpu.ETI_READ_FP_BREAK,
                                                 dabgpu.ETI_READ_ERR_FIELD, dabgpu.ETI_READ_FIB_CRC] == \
        [RR.BAD_DATA_CRC, RR.OTHER_PLAN, RR.GAP, RR.FP_BREAK, RR.ERR_FIELD, RR.FIB_CRC]


def test_state_record_size(built):
    assert dabgpu.eti_read_state_bytes() == STATE_BYTES == dabgpu.ETI_READ_HEAD_DTYPE.itemsize + 6144 and STATE_BYTES % 16 == 0
    assert "dabgpu_eti_read_dev" in dabgpu.EXPORTS and dabgpu.lib().dabgpu_abi_version() == 6


@pytest.fixture(scope="module")
def damaged():
    return {name: damage_set(name, 10 + 2 * i) for i, name in enumerate(CONFIGS)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_host_twin_equals_the_reference_on_damaged_streams(built, damaged, name):
    data, ref = damaged[name]
    case = Case(CONFIGS[name](), data)
    got = run_host([case])[0]
    rows, result, new = assert_is_reference(case, got, what=name)
    # the reference itself has met everything: every verdict, a resync, a gap, a tail
    assert {r["verdict"] for r in rows} == {0, 4, 5} and result["resyncs"] >= 5 and result["gap_sum"] > 0 and result["tail_bytes"] > 0
    assert any(r["flags"] & RR.FIB_CRC for r in rows) and any(r["flags"] & RR.FP_BREAK for r in rows)
    assert any(r["flags"] & RR.ERR_FIELD for r in rows)
    # verdict consistency: every row's verdict is dabgpu_eti_parse's on those bytes, or 5 where it says 0 and the plan differs
    plan = dabgpu.eti_layout(CONFIGS[name]())
    for r in range(int(got["result"]["rows"])):
        st = got["status"][r]
        frame = np.frombuffer(data[int(st["offset"]):int(st["offset"]) + FRAME], np.uint8)
        info = dabgpu.EtiInfo()
        rc = dabgpu.lib().dabgpu_eti_parse(frame.ctypes.data, C.byref(info))
        differs = info.nst != plan.nst or info.fl != plan.fl or bytes(frame[8:8 + 4 * info.nst]) != bytes(plan.header[8:8 + 4 * plan.nst])
        assert int(st["verdict"]) == (5 if rc == 0 and differs else rc), (r, rc, st)


@pytest.mark.parametrize("name", ["full_cif", "fic_only"])
def test_host_twin_sees_a_flip_in_each_of_the_64_crc_chunks(built, name):
    frames, ref = make_frames(name, 2, 5)
    data = b"".join(chunk_flips(frames[1], ref)) + frames[0]
    case = Case(CONFIGS[name](), data)
    got = run_host([case])[0]
    assert list(got["status"]["verdict"][:65]) == [4] * 64 + [0] and int(got["result"]["rows"]) == 65
    if name == "fic_only":                                   # (the reference's CRC is slow on 64 full frames: the small one only)
        assert_is_reference(case, got)


def test_discovery_pass_and_unwanted_streams(built, damaged):
    data, ref = damaged["uep_and_eep_b"]
    streams = CONFIGS["uep_and_eep_b"]()
    none, some = Case(None, data), Case(streams, data, wanted=[True, False, True])
    a, b = run_host([none, some])
    rows, _, _ = assert_is_reference(none, a)
    assert_is_reference(some, b)
    assert 5 not in {r["verdict"] for r in rows}
    # the multiplex is read from a taken frame at the offset its status gives
    at = int(a["status"][0]["offset"])
    found = dabgpu.eti_streams(data[at:at + FRAME])
    assert sorted((s.subchannel_id, s.sc.start_address, s.sc.bitrate_kbps) for s in found) == \
        sorted((i, sc.start_address, sc.bitrate_kbps) for i, sc in streams)


def _without_offsets(status):
    st = status.copy()
    st["offset"] = 0
    return st.tobytes()


def _two_calls(streams, data, cut):
    first = run_host([Case(streams, data[:cut])])[0]
    second = run_host([Case(streams, data[cut:], state=first["state"])])[0]
    return first, second


def _joined(first, second):
    n1, n2 = int(first["result"]["rows"]), int(second["result"]["rows"])
    st = np.concatenate([first["status"][:n1], second["status"][:n2]])
    return {"fib": np.concatenate([first["fib"][:n1], second["fib"][:n2]]), "crc_ok": np.concatenate([first["crc_ok"][:n1], second["crc_ok"][:n2]]),
            "outs": [np.concatenate([x[:n1], y[:n2]]) for x, y in zip(first["outs"], second["outs"])],
            "status": _without_offsets(st), "state": second["state"]}


def assert_cut_equals_whole(streams, data, cuts):
    whole = run_host([Case(streams, data)])[0]
    n = int(whole["result"]["rows"])
    want = {"fib": whole["fib"][:n], "crc_ok": whole["crc_ok"][:n], "outs": [o[:n] for o in whole["outs"]],
            "status": _without_offsets(whole["status"][:n]), "state": whole["state"]}
    for cut in cuts:
        first, second = _two_calls(streams, data, cut)
        got = _joined(first, second)
        # (a row's offset counts from the start of ITS call's S: everything else is the same, and so is the final state)
        assert got["status"] == want["status"] and got["fib"].tobytes() == want["fib"].tobytes(), cut
        assert got["crc_ok"].tobytes() == want["crc_ok"].tobytes() and got["state"].tobytes() == want["state"].tobytes(), cut
        for x, y in zip(got["outs"], want["outs"]):
            assert x.tobytes() == y.tobytes(), cut


def test_cut_at_every_byte_of_three_frames(built):
    frames, _ = make_frames("tiny", 3, 3, start=248)
    data = b"".join(frames)
    assert_cut_equals_whole(CONFIGS["tiny"](), data, range(len(data) + 1))


@pytest.mark.parametrize("name", ["uep_and_eep_b", "multiplex18"])
def test_random_cuts_of_damaged_streams(built, damaged, name):
    data, _ = damaged[name]
    rng = np.random.default_rng(4)
    assert_cut_equals_whole(CONFIGS[name](), data, [int(x) for x in rng.integers(0, len(data) + 1, 40)] + [6143, 6144, 6145])


def test_many_pieces_equal_one_call(built, damaged):
    data, _ = damaged["one_eep_a"]
    streams = CONFIGS["one_eep_a"]()
    rng = np.random.default_rng(6)
    whole = run_host([Case(streams, data)])[0]
    state, at, rows, ref_state = None, 0, 0, None
    while at < len(data):
        n = int(rng.choice([0, 1, 15, 500, 6143, 6144, 6145, 20000]))
        case = Case(streams, data[at:at + n], state=state)
        got = run_host([case])[0]
        _, _, ref_state = assert_is_reference(case, got, state=ref_state, what="piece at %d" % at)
        state, at, rows = got["state"], at + n, rows + int(got["result"]["rows"])
    assert rows == int(whole["result"]["rows"]) and state.tobytes() == whole["state"].tobytes()


@pytest.mark.parametrize("n", [0, 1, 6143, 6144, 6145])
def test_edge_sizes(built, n):
    frames, _ = make_frames("one_eep_a", 2, 7)
    data = b"".join(frames)
    for start in (0, 1):
        case = Case(CONFIGS["one_eep_a"](), data[start:start + n])
        got = run_host([case])[0]
        rows, result, _ = assert_is_reference(case, got, what=(n, start))
        assert len(rows) == (1 if n >= 6144 and start == 0 else 0) and result["tail_bytes"] == (n - 6144 * len(rows) if n < 6144 or start == 0 else 6143)


def test_hostile_state_is_clamped(built):
    frames, _ = make_frames("tiny", 2, 9)
    data = b"".join(frames)
    hostile = np.full(STATE_BYTES, 0xFF, np.uint8)
    case = Case(CONFIGS["tiny"](), data, state=hostile)
    got = run_host([case])[0]
    # what the record stands for: a tail of 6143 bytes 0xFF, a previous row with FCT 255 and FP 255, totals of all ones
    state = {"tail": b"\xff" * 6143, "have_prev": True, "last_fct": 255, "last_fp": 255, "totals": dict.fromkeys(RR.COUNTERS, 2 ** 64 - 1)}
    rows, result, new = RR.read(state, data, [ref_stream(i, sc) for i, sc in CONFIGS["tiny"]()])
    assert int(got["result"]["rows"]) == len(rows) == 2 and int(got["result"]["skipped"]) == 6143
    assert [int(got["status"][r]["offset"]) for r in range(2)] == [6143, 6143 + 6144]
    assert int(got["status"][0]["gap"]) == rows[0]["gap"] and int(got["status"][0]["flags"]) == rows[0]["flags"]
    head = got["state"][:80].view(dabgpu.ETI_READ_HEAD_DTYPE)[0]
    assert int(head["rows"]) == (2 ** 64 - 1 + 2) % 2 ** 64 and int(head["tail_bytes"]) == 0
    # a record of zeros with a hostile length only: the tail is the record's own (zero) bytes, nothing outside it
    zeros = np.zeros(STATE_BYTES, np.uint8)
    zeros[:4] = 0xFF
    got = run_host([Case(CONFIGS["tiny"](), data, state=zeros)])[0]
    assert int(got["result"]["rows"]) == 2 and int(got["result"]["skipped"]) == 6143


def test_refused_calls_write_nothing(built):
    frames, _ = make_frames("tiny", 2, 11)
    case = Case(CONFIGS["tiny"](), b"".join(frames), state=np.zeros(STATE_BYTES, np.uint8))
    run_host([case])                                          # (sets the arrays up)
    a = case.arrays
    for k in ("fib", "crc_ok", "status", "result", "state_out"):
        a[k][:] = FILL
    a["outs"][0][:] = FILL
    keep = []
    addr = lambda x: x.ctypes.data

    def entry(**kw):
        e = _entry(case, addr, keep)
        for k, v in kw.items():
            setattr(e, k, v)
        return e
    bad_plan = dabgpu.eti_layout(CONFIGS["tiny"]())
    bad_plan.bytes[0] = 48
    bad_out = (C.c_void_p * 1)(addr(a["outs"][0]) + 4)
    good = entry()
    for bad in (entry(d_bytes=addr(a["bytes"]) + 8), entry(d_state_out=addr(a["state_in"])), entry(n_bytes=-1),
                entry(d_state_out=addr(a["state_out"]) + 8), entry(d_state_in=addr(a["state_in"]) + 4), entry(d_status=addr(a["status"]) + 4),
                entry(plan=C.pointer(bad_plan)), entry(d_out=C.cast(bad_out, C.POINTER(C.c_void_p))), entry(d_result=None)):
        for entries in ([bad], [good, bad]):
            with pytest.raises(dabgpu.DabGpuError) as e:
                dabgpu.eti_read_host(entries)
            assert e.value.status == -1
    arr = (dabgpu.EtiReadEntry * 1)(good)
    assert dabgpu.lib().dabgpu_eti_read_host(arr, -1) == -1 and dabgpu.lib().dabgpu_eti_read_host(None, 1) == -1
    for k in ("fib", "crc_ok", "status", "result", "state_out"):
        assert (a[k] == FILL).all(), k
    assert (a["outs"][0] == FILL).all()


def _build_and_run(tmp_path, source, flags, args=()):
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", source), "-o", exe])
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)


def test_fuzz_the_walk_under_sanitizers(tmp_path):
    """tests/eti_read_fuzz.cpp: the header alone, compiled with -fsanitize=address,undefined into its own program, on random
    and mutated streams and states."""
    p = _build_and_run(tmp_path, "eti_read_fuzz.cpp", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["300"])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "ok" in p.stdout


def test_kernels_use_no_scratch_and_spill_nothing(built, tmp_path):
    from test_device_asm import kernel_metadata
    csrc = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "csrc")
    obj, tools = os.path.join(csrc, "eti_read_kernels.o"), "/opt/rocm/lib/llvm/bin/"
    if not os.path.exists(obj):
        subprocess.check_call(["make", "-C", csrc, "eti_read_kernels.o"], stdout=subprocess.DEVNULL)
    fat, co = str(tmp_path / "eti_read.fat"), str(tmp_path / "eti_read.co")
    subprocess.check_call([tools + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([tools + "clang-offload-bundler", "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    md = kernel_metadata(subprocess.check_output([tools + "llvm-readelf", "--notes", co], text=True))
    assert sorted(k.split("eti_read_")[1].split("_kernel")[0] for k in md) == ["chain", "finish", "row", "scan"], list(md)
    for k, v in md.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v.get("agpr_count", 0) == 0 and v["vgpr_count"] <= 64, (k, v)              # 8 waves per SIMD
    row = [v for k, v in md.items() if "eti_read_row_kernel" in k][0]
    assert row["group_segment_fixed_size"] <= 160 * 1024 // 6                             # four frames in LDS: six workgroups per CU


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def rctx(built):
    c = make_ctx(None, max_frames=64)
    yield c
    c.close()


def assert_device_is_host(ctx, make_cases, what=""):
    host_cases, dev_cases = make_cases(), make_cases()
    want, got = run_host(host_cases), run_dev(ctx, dev_cases)
    for i, (w, g) in enumerate(zip(want, got)):
        assert_same(g, w, "%s entry %d" % (what, i))
    return want


@pytest.mark.gpu
def test_device_five_plans_in_one_call_with_damage(rctx, damaged):
    names = ["fic_only", "tiny", "uep_and_eep_b", "multiplex18", "full_cif"]
    want = assert_device_is_host(rctx, lambda: [Case(CONFIGS[n](), damaged[n][0]) for n in names])
    for w in want:
        assert set(w["status"]["verdict"][:int(w["result"]["rows"])]) == {0, 4, 5} and int(w["result"]["resyncs"]) >= 5


@pytest.mark.gpu
def test_device_row_counts_across_the_seams(rctx):
    counts = [1, 3, 4, 5, 63, 64, 65]
    frames = {n: make_frames(n, 65, 21 + i)[0] for i, n in enumerate(("tiny", "uep_and_eep_b"))}
    want = assert_device_is_host(rctx, lambda: [Case(CONFIGS[n](), b"".join(frames[n][:k])) for k in counts for n in frames])
    assert [int(w["result"]["rows"]) for w in want] == [k for k in counts for _ in frames]


@pytest.mark.gpu
def test_device_257_frames_of_one_entry(rctx):
    frames, _ = make_frames("tiny", 257, 31)
    data = b"".join(frames)
    data = data[:100 * 6144 + 77] + data[100 * 6144 + 99:]    # and a resync far into the bitmap
    want = assert_device_is_host(rctx, lambda: [Case(CONFIGS["tiny"](), data)])
    assert int(want[0]["result"]["rows"]) == 256 and int(want[0]["result"]["resyncs"]) == 1


@pytest.mark.gpu
def test_device_streams_that_start_inside_a_frame(rctx):
    frames, _ = make_frames("uep_and_eep_b", 6, 41)
    data = b"".join(frames)
    offsets = [0, 1, 15, 16, 6143]
    want = assert_device_is_host(rctx, lambda: [Case(CONFIGS["uep_and_eep_b"](), data[o:]) for o in offsets])
    assert [int(w["result"]["rows"]) for w in want] == [6, 5, 5, 5, 5]
    assert [int(w["result"]["skipped"]) for w in want] == [0, 6143, 6129, 6128, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["full_cif", "fic_only"])
def test_device_sees_a_flip_in_each_of_the_64_crc_chunks(rctx, name):
    frames, ref = make_frames(name, 2, 5)
    data = b"".join(chunk_flips(frames[1], ref)) + frames[0]
    want = assert_device_is_host(rctx, lambda: [Case(CONFIGS[name](), data), Case(None, data)])
    for w in want:
        assert list(w["status"]["verdict"][:65]) == [4] * 64 + [0]


@pytest.mark.gpu
def test_device_unwanted_streams_and_discovery(rctx, damaged):
    data = damaged["multiplex18"][0]
    wanted = [k % 3 != 1 for k in range(18)]
    assert_device_is_host(rctx, lambda: [Case(CONFIGS["multiplex18"](), data, wanted=wanted), Case(None, data),
                                         Case(CONFIGS["multiplex18"](), data, wanted=[False] * 18), Case(CONFIGS["tiny"](), b"")])


@pytest.mark.gpu
def test_device_two_calls_with_the_carry_equal_the_host_twins(rctx, damaged):
    names = ["uep_and_eep_b", "full_cif", "tiny"]
    cuts = {"uep_and_eep_b": 6144 * 9 + 3001, "full_cif": 6143, "tiny": 6144 * 17 + 50}
    first = assert_device_is_host(rctx, lambda: [Case(CONFIGS[n](), damaged[n][0][:cuts[n]]) for n in names], "first")
    hostile = np.full(STATE_BYTES, 0xFF, np.uint8)
    assert_device_is_host(rctx, lambda: [Case(CONFIGS[n](), damaged[n][0][cuts[n]:], state=f["state"]) for n, f in zip(names, first)] +
                          [Case(CONFIGS["tiny"](), damaged["tiny"][0][:20000], state=hostile)], "second")


@pytest.mark.gpu
def test_device_refused_calls_write_nothing(rctx):
    import torch
    frames, _ = make_frames("tiny", 2, 11)
    case = Case(CONFIGS["tiny"](), b"".join(frames), state=np.zeros(STATE_BYTES, np.uint8))
    run_dev(rctx, [case])
    a = case.arrays
    for k in ("fib", "crc_ok", "status", "result", "state_out"):
        a[k].fill_(FILL)
    a["outs"][0].fill_(FILL)
    torch.cuda.synchronize()
    keep = []
    addr = lambda x: x.data_ptr()

    def entry(**kw):
        e = _entry(case, addr, keep)
        for k, v in kw.items():
            setattr(e, k, v)
        return e
    for bad in (entry(d_bytes=addr(a["bytes"]) + 8), entry(d_state_out=addr(a["state_in"])), entry(n_bytes=-1),
                entry(d_fib=addr(a["fib"]) + 4), entry(d_state_in=addr(a["state_in"]) + 8)):
        with pytest.raises(dabgpu.DabGpuError) as e:
            rctx.eti_read_dev([entry(), bad])
        assert e.value.status == -1
    rctx.sync()
    for k in ("fib", "crc_ok", "status", "result", "state_out"):
        assert bool((a[k] == FILL).all()), k
    assert bool((a["outs"][0] == FILL).all())


@pytest.mark.gpu
def test_round_trip_through_the_writer(rctx):
    """Random d_fib, d_crc_ok and d_out through dabgpu_eti_frames_dev, then through the reader: the same sub-channel bytes,
    the FIC 15 CIFs late, the CRC flags wherever the FIB really carries a right CRC."""
    import torch
    from test_eti import run_eti
    rng = np.random.default_rng(51)
    streams = CONFIGS["uep_and_eep_b"]()
    n_streams, n_cif = 3, 32
    fib = np.zeros((n_streams, n_cif, 3, 32), np.uint8)
    ok = np.zeros((n_streams, n_cif, 3), np.uint8)
    for s in range(n_streams):
        fib[s], ok[s] = make_fibs(rng, n_cif, bad_every=5 + s)
    claimed = ok.copy()
    claimed[0, 20] ^= 1                                       # flags that do not say what the bytes say
    outs = [rng.integers(0, 256, (n_streams, n_cif, sc.bitrate_kbps * 3), dtype=np.uint8) for _, sc in streams]
    eti, _, _ = run_eti(rctx, streams, fib, claimed, outs)
    got_fib, got_ok, got_outs, status, result, _ = rctx.eti_read(torch.from_numpy(eti.reshape(n_streams, -1)).cuda(), streams)
    res = result.cpu().numpy().view(dabgpu.ETI_READ_RESULT_DTYPE).reshape(-1)
    assert (res["rows"] == n_cif).all() and (res["taken"] == n_cif).all() and not res["skipped"].any() and not res["tail_bytes"].any()
    for k in range(len(streams)):
        assert got_outs[k].cpu().numpy().tobytes() == outs[k].tobytes()
    got_fib, got_ok = got_fib.cpu().numpy(), got_ok.cpu().numpy()
    assert not got_fib[:, :15].any() and got_fib[:, 15:].tobytes() == fib[:, :n_cif - 15].tobytes()
    assert got_ok[:, 15:].tobytes() == ok[:, :n_cif - 15].tobytes()
    st = status.cpu().numpy().view(dabgpu.ETI_READ_STATUS_DTYPE).reshape(n_streams, n_cif)
    assert not st["gap"].any() and not (st["flags"] & (dabgpu.ETI_READ_GAP | dabgpu.ETI_READ_FP_BREAK)).any()
    assert (st["flags"][:, :15] & dabgpu.ETI_READ_ERR_FIELD).all()


@pytest.mark.gpu
def test_follow_call_on_the_readers_rows(rctx):
    """dabgpu_dabplus_follow_dev finds the same super-frames on the reader's d_out as on the buffers that went into the writer."""
    import torch
    from test_eti import SERVICES, run_eti
    ens = synth.ServiceEnsemble(7, SERVICES[:1], n_frames=10, extras=False)
    streams = [(3, dabgpu.subchannel(0, 64, level=3))]
    lf = np.ascontiguousarray(np.asarray(ens.msc_bytes[0], np.uint8)[:40]).reshape(1, 40, 192)
    fib, ok = make_fibs(np.random.default_rng(1), 40)
    eti, _, _ = run_eti(rctx, streams, fib[None], ok[None], [lf])
    _, _, outs, _, result, _ = rctx.eti_read(torch.from_numpy(eti.reshape(1, -1)).cuda(), streams)

    def follow(d_in):
        z = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")
        carry, data, status, res = z(dabgpu.dabplus_carry_bytes(64)), z(8 * 110 * 8), z(8 * 64), z(32)
        rctx.dabplus_follow_dev([dabgpu.DabplusEntry(d_in.data_ptr(), 192, 64, None, carry.data_ptr(), data.data_ptr(), status.data_ptr(),
                                                     res.data_ptr())], 40)
        rctx.sync()
        return data.cpu().numpy(), status.cpu().numpy(), res.cpu().numpy().view(dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)[0], carry.cpu().numpy()
    a = follow(torch.from_numpy(lf.reshape(40, 192)).cuda())
    b = follow(outs[0].reshape(40, 192))
    assert int(a[2]["n_superframes"]) >= 1 and a[2].tobytes() == b[2].tobytes()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes()


# ------------------------------------------------------------------ the host mirror
HOST = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")


def test_mirror_reads_an_eti_stream_in_uneven_pieces(built, tmp_path):
    """tests/eti_read_mirror_check.cpp: BasicRadio::ProcessEti over the TEST-ONLY fake ABI (unchanged: the walk is the header's,
    no new symbol).  Three cycles of a synthetic ensemble -- a DAB+ service with a dynamic label, a layer-II service, a
    packet-mode component -- as ETI from the reference writer, fed in uneven pieces: the services, the label and the counts the
    transmit side gives.  The channels exist once the first frame's FIC is parsed, so they are fed from the second frame on."""
    import test_mp2_end_to_end as E
    import test_packet as P
    fake, oracle = os.path.join(ROOT, "tests", "fake_abi"), os.path.join(ROOT, "oracle")
    assert "eti_read" not in open(os.path.join(fake, "fake_dabgpu.cpp")).read()
    exe = str(tmp_path / "eti_read_mirror_check")
    srcs = [os.path.join(ROOT, "tests", "eti_read_mirror_check.cpp"), os.path.join(fake, "fake_dabgpu.cpp")]
    srcs += [os.path.join(HOST, s) for s in ("ofdm/ofdm_demodulator.cpp", "basic_radio/basic_radio.cpp", "basic_radio/basic_dab_plus_channel.cpp", "dab/fic/fic_parser.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), "-I" + oracle, "-I" + fake] + srcs +
                          ["-L" + oracle, "-loracle", "-Wl,-rpath," + oracle, "-o", exe])
    _pe, frames = P.e2e_ensemble()
    service = ("Slides", 0xD301, P.E2E_SUBCH, 0, 3, 32, P.E2E_START, [(P.E2E_SCID, P.ADDR, synth.DSCTY_MOT, 0)], frames, 0)
    bodies, _plain = E.dabplus_bodies()
    ens = synth.ServiceEnsemble(E.SEED, E.SERVICES, n_frames=5, dab_services=E.DAB, extras=False, bodies=bodies, dab_pads=[E.mp2_pads()],
                                packet_services=[service])
    streams = [{"id": 3, "start": 0, "bitrate": 64, "uep": False, "eep_type": 0, "level": 3},
               {"id": P.E2E_SUBCH, "start": P.E2E_START, "bitrate": 32, "uep": False, "eep_type": 0, "level": 3},
               ref_stream(11, dabgpu.uep_subchannel(17, 100))]
    fibs = ens.fibs.reshape(20, 96)
    sent = {3: ens.msc_bytes[0], P.E2E_SUBCH: frames, 11: ens.mp2_frames[0]}
    eti = b"".join(R.write_frame(streams, c, fibs[c % 20].tobytes(), {i: bytes(d[c % 20]) for i, d in sent.items()}, 0xFF) for c in range(60))
    cut = eti[:45 * 6144 + 1000] + eti[45 * 6144 + 1100:]                      # ... and once more with 100 bytes lost in frame 45

    def run(data, pieces):
        path = tmp_path / "in.eti"
        path.write_bytes(data)
        r = subprocess.run([exe, str(path)] + [str(p) for p in pieces], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return {l.split()[0] + (" " + l.split()[1] if l.split()[0] in ("channel", "packet", "service") else ""): dict(kv.split("=", 1) for kv in l.split()[1:])
                for l in r.stdout.splitlines()}
    out = run(eti, [1, 5000, 6143, 17, 20000, 6145])
    read = {k: int(v) for k, v in out["read"].items()}
    assert (read["rows"], read["taken"], read["skipped"], read["resyncs"], read["gap_sum"], read["fib_errors"], read["tail"], read["fibs"]) == \
        (60, 60, 0, 0, 0, 0, 0, 180), read
    assert bytes.fromhex(out["ensemble"]["label"]).rstrip() == b"Synth Ensemble"
    assert sorted(bytes.fromhex(out[k]["label"]).rstrip() for k in out if k.startswith("service")) == [b"Classic", b"Radio One", b"Slides"]
    plus, mp2, packet = out["channel subchannel=3"], out["channel subchannel=11"], out["packet subchannel=%d" % P.E2E_SUBCH]
    per_sf = [len(a) for a in ens.aus[0]]                                      # access units per super-frame of the cycle
    assert int(plus["superframes"]) == 11 and int(plus["aus"]) == int(plus["handed"]) == 3 * sum(per_sf) - per_sf[0] and plus["au_errors"] == "0"
    assert bytes.fromhex(plus["label"]) == E.LABELS[0]
    assert (int(mp2["mp2_frames"]), int(mp2["handed"]), mp2["header_errors"], mp2["crc_errors"]) == (59, 59, "0", "0")
    assert bytes.fromhex(mp2["label"]) == E.LABELS[1]
    assert (int(packet["frames"]), packet["addresses"], packet["objects"]) == (59, "1", "1")
    out = run(cut, [7001, 3])
    read = {k: int(v) for k, v in out["read"].items()}
    assert (read["rows"], read["taken"], read["skipped"], read["resyncs"], read["gap_sum"], read["tail"]) == (59, 59, 6044, 1, 1, 0), read
    assert int(out["channel subchannel=11"]["mp2_frames"]) == 58
