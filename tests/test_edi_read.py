"""EDI input (include/dabgpu.h, "EDI input"; include/dabgpu_edi.h, "THE CONTRACT"): AF packet byte streams read back into
FIBs, CRC flags and logical frames.  The host call is held byte for byte to tests/edi_read_reference.py (the contract in plain
Python) -- rows, status, result and state; outputs start out as 0xEE so that what a call must not write is compared too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dabgpu
import edi_read_reference as RR
import edi_reference as P
import eti_reference as R
from conftest import ROOT
from dabgpu import synth
from test_eti import CONFIGS, ref_stream
from test_eti_read import aligned, flip, make_fibs

HEAD = 96
STATE_BYTES = HEAD + 8192
FILL = 0xEE
COUNTERS = ("rows", "not_deti", "bad_tags", "other_plan", "skipped", "resyncs", "gap_sum", "fib_errors")


# ------------------------------------------------------------------ streams and damage
def make_packets(name, n_cif, seed, start=0, seq=0):
    """n_cif packets of configuration `name` from the reference writer -> (list of packets, stream dicts)."""
    rng = np.random.default_rng(seed)
    ref = [ref_stream(i, sc) for i, sc in CONFIGS[name]()]
    fibs, ok = make_fibs(rng, n_cif)
    data = {st["id"]: rng.integers(0, 256, (n_cif, st["bitrate"] * 3), dtype=np.uint8) for st in ref}
    hist = {"fibs": [fibs[0]] * 15, "crc_ok": [ok[0]] * 15, "next_count": start} if seed % 2 else None   # odd seeds: no warm-up
    stream, _, _ = P.write_stream(ref, fibs, ok, data, history=hist, cif_start=start, seq_start=seq)
    n = P.packet_bytes(ref)
    return [stream[i * n:(i + 1) * n] for i in range(n_cif)], ref


def recrc(p):
    return p[:-2] + synth.crc16(p[:-2]).to_bytes(2, "big")


def nested_pair(seed=3):
    """(intact, broken): a one_eep_a packet whose sub-channel data hold a complete valid FIC-only packet; broken has the
    outer CRC wrong, so the inner one is found."""
    outer, ref = make_packets("one_eep_a", 1, seed, start=700, seq=50)
    inner, _ = make_packets("fic_only", 1, seed + 1, start=4321, seq=9)
    at = 136 + 11 + 20
    assert len(inner[0]) == 140 and at + 140 <= len(outer[0]) - 2
    intact = recrc(outer[0][:at] + inner[0] + outer[0][at + 140:])
    return intact, flip(intact, len(intact) - 1, 2), inner[0]


def damage_set(name, seed):
    """A stream of configuration `name` with every kind of damage, as one byte string, and its stream dicts."""
    pk, ref = make_packets(name, 40, seed, start=4980, seq=65522)            # packet t: dlfc 4965 + t, SEQ 65522 + t
    n = len(pk[0])
    data0 = {st["id"]: bytes(st["bitrate"] * 3) for st in ref}
    f = list(pk)
    f[2] = flip(f[2], 3, 1)                                   # header: LEN
    f[3] = flip(f[3], 7, 0)                                   # header: SEQ (the CRC fails)
    f[4] = flip(f[4], 60, 5)                                  # payload
    f[6] = flip(f[6], n - 1, 3)                               # CRC
    f[8] = f[8][:100] + f[8][101:]                            # 1 byte gone
    f[9] = f[9][:17] + f[9][34:]                              # 17 bytes gone
    f[11] = f[11][:50] + b"\x01\x02\x03\x04\x05" + f[11][50:]  # 5 bytes too many
    f[13] += P.af_packet(P.item("*dmy", bytes(24)), 7)         # foreign packets between: only *dmy ...
    f[14] += P.af_packet(P.PTR_DETI + P.item("abcd", bytes(9)), 8)   # ... PT-valid without deti
    other, _ = make_packets("tiny" if name != "tiny" else "one_eep_a", 1, seed + 2, start=17, seq=1000)
    f[16] = other[0]                                          # a packet of another plan
    f[18] = P.write_packet(ref, 4965 + 18, 65522 + 18, None, data0, 0xFF, time=(37, 0x5EED5EED, 0x123456))   # ATSTF = 1, FICF = 0
    f[19] = P.write_packet(ref, 4965 + 19, 65522 + 19, bytes(f[19][40:136]), data0, 0xE1, time=(37, 1, 2), fp=5)
    f[21] = P.af_packet(P.item("deti", b"\x40\x00\xff"), 77)   # malformed: a deti of 24 bits
    f[23] = b"AF" + (3 * n).to_bytes(4, "big") + b"\0\0\x90T" + f[23]     # a plausible header with a wrong LEN in front
    del f[26:29]                                              # a dlfc jump
    if name in ("one_eep_a", "multiplex18", "uep_and_eep_b", "full_cif"):
        intact, broken, _ = nested_pair()
        f[28] += intact if name != "one_eep_a" else b""
        f[29] += broken if name != "one_eep_a" else b""
        if name == "one_eep_a":                               # ... of this very plan: rows
            f[28], f[29] = intact, broken
    f[-1] = f[-1][:n - 7]                                     # the stream ends inside a packet
    return b"".join(f), ref


# ------------------------------------------------------------------ running the call
class Case:
    """One entry: plan streams [(scid, Subchannel)] or None, the new bytes, the state record (uint8 [STATE_BYTES]) or None,
    which streams are wanted (None: all)."""

    def __init__(self, streams, data, state=None, wanted=None):
        self.streams, self.data, self.state, self.wanted = streams, bytes(data), state, wanted
        self.plan = None if streams is None else dabgpu.eti_layout(streams)
        self.rows = dabgpu.edi_read_max_rows(len(self.data), self.plan)
        self.sizes = [] if streams is None else [sc.bitrate_kbps * 3 for _, sc in streams]
        if wanted is None:
            self.wanted = [True] * len(self.sizes)


def _entry(case, addr, keep):
    a = case.arrays
    ptrs = (C.c_void_p * max(len(case.sizes), 1))(*[addr(o) if w else 0 for o, w in zip(a["outs"], case.wanted)])
    keep.append(ptrs)
    return dabgpu.EdiReadEntry(addr(a["bytes"]) if len(case.data) else None, len(case.data), 0,
                               C.pointer(case.plan) if case.plan is not None else None,
                               C.cast(ptrs, C.POINTER(C.c_void_p)) if case.plan is not None else None,
                               None if a["state_in"] is None else addr(a["state_in"]), addr(a["state_out"]), addr(a["fib"]),
                               addr(a["crc_ok"]), addr(a["status"]), addr(a["result"]))


def _collect(case, get):
    a = case.arrays
    return {"fib": get(a["fib"]).reshape(-1, 96), "crc_ok": get(a["crc_ok"]).reshape(-1, 3),
            "outs": [get(o).reshape(case.rows, -1) for o in a["outs"]],
            "status": get(a["status"]).view(dabgpu.EDI_READ_STATUS_DTYPE).reshape(-1),
            "result": get(a["result"]).view(dabgpu.EDI_READ_RESULT_DTYPE)[0], "state": get(a["state_out"])}


def host_entries(cases):
    keep, entries = [], []
    for c in cases:
        c.arrays = {"bytes": aligned(max(len(c.data), 1)), "state_in": None, "state_out": aligned(STATE_BYTES),
                    "fib": aligned(c.rows * 96), "crc_ok": aligned(c.rows * 3), "status": aligned(c.rows * 32),
                    "result": aligned(48), "outs": [aligned(c.rows * n) for n in c.sizes]}
        c.arrays["bytes"][:len(c.data)] = np.frombuffer(c.data, np.uint8)
        if c.state is not None:
            c.arrays["state_in"] = aligned(STATE_BYTES)
            c.arrays["state_in"][:] = c.state
        entries.append(_entry(c, lambda x: x.ctypes.data, keep))
    return entries, keep


def run_host(cases):
    entries, keep = host_entries(cases)
    dabgpu.edi_read_host(entries)
    return [_collect(c, lambda x: x.copy()) for c in cases]


def state_of_record(rec):
    """a record the library wrote (or None) -> the reference's state"""
    if rec is None:
        return RR.new_state()
    h = rec[:HEAD].view(dabgpu.EDI_READ_HEAD_DTYPE)[0]
    n = min(int(h["tail_bytes"]), 8191)
    return {"tail": rec[HEAD:HEAD + n].tobytes(), "prev": int(h["last_dlfc"]) % 5000 if h["have_prev"] else None,
            "seq": int(h["last_seq"]) if h["have_seq"] else None, "in_skip": bool(h["in_skip"])}


def assert_is_reference(case, got, what=""):
    """the host call's outputs of one case against the reference reader"""
    plan = None if case.streams is None else [ref_stream(i, sc) for i, sc in case.streams]
    order = None if plan is None else [[st["id"] for st in R.ordered(plan)].index(i) for i, _ in case.streams]
    rows, result, new = RR.read(state_of_record(case.state), case.data, plan)
    res = got["result"]
    assert {k: int(res[k]) for k in COUNTERS + ("tail_bytes",)} == result, (what, res, result)
    assert not res["reserved"].any()
    n = len(rows)
    assert n <= case.rows
    for r, row in enumerate(rows):
        st, want = got["status"][r], row["status"]
        assert {k: int(st[k]) for k in want} == want, (what, r, st, want)
        assert not st["reserved"].any() and int(st["reserved2"]) == 0
        assert got["fib"][r].tobytes() == row["fic"] and list(got["crc_ok"][r]) == row["crc_ok"], (what, r)
        for k in range(len(case.sizes)):
            if case.wanted[k]:
                assert got["outs"][k][r].tobytes() == row["data"][order[k]], (what, r, k)
    # nothing behind the emitted rows, and nothing for a stream that is not wanted
    assert (got["fib"][n:] == FILL).all() and (got["crc_ok"][n:] == FILL).all() and (got["status"].view(np.uint8)[32 * n:] == FILL).all()
    for k, o in enumerate(got["outs"]):
        assert (o[n if case.wanted[k] else 0:] == FILL).all()
    head = got["state"][:HEAD].view(dabgpu.EDI_READ_HEAD_DTYPE)[0]
    assert state_of_record(got["state"]) == new, what
    assert int(head["tail_bytes"]) == len(new["tail"]) == result["tail_bytes"] and not got["state"][HEAD + len(new["tail"]):].any()
    assert int(head["reserved"]) == 0 and int(head["reserved1"]) == 0 and not head["reserved2"].any()
    before = None if case.state is None else case.state[:HEAD].view(dabgpu.EDI_READ_HEAD_DTYPE)[0]
    for k in COUNTERS:
        assert int(head[k]) == (0 if before is None else int(before[k])) + result[k], (what, k)
    return rows, result, new


# ------------------------------------------------------------------ CPU
@pytest.fixture(scope="module")
def damaged():
    return {name: damage_set(name, 10 + 2 * i) for i, name in enumerate(CONFIGS)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_host_call_equals_the_reference_on_damaged_streams(built, damaged, name):
    data, ref = damaged[name]
    case = Case(CONFIGS[name](), data)
    got = run_host([case])[0]
    rows, result, new = assert_is_reference(case, got, what=name)
    # the reference itself has met everything
    assert result["resyncs"] >= 5 and result["gap_sum"] > 0 and result["tail_bytes"] > 0 and result["skipped"] > 0
    assert result["not_deti"] >= 2 and result["bad_tags"] >= 1 and result["other_plan"] >= 1 and result["fib_errors"] > 0
    flags = [r["status"]["flags"] for r in rows]
    for bit in (RR.GAP, RR.SEQ_BREAK, RR.FP_MISMATCH, RR.STAT_FIELD, RR.FIB_CRC, RR.NO_FIC, RR.TIME):
        assert any(f & bit for f in flags), bit
    assert any(r["status"]["dlfc"] == 4999 for r in rows) and any(r["status"]["dlfc"] == 0 for r in rows)
    assert any(r["status"]["seq"] == 65535 for r in rows) and any(r["status"]["seq"] == 0 for r in rows)
    timed = [r["status"] for r in rows if r["status"]["flags"] & RR.NO_FIC]
    assert (timed[0]["utco"], timed[0]["seconds"], timed[0]["tsta"]) == (37, 0x5EED5EED, 0x123456)
    # every row's packet is one dabgpu_edi_parse passes, of the plan
    for r in range(int(got["result"]["rows"])):
        st = got["status"][r]
        info = dabgpu.edi_parse(data[int(st["offset"]):int(st["offset"]) + int(st["length"])])
        assert info["dlfc"] == st["dlfc"] and info["seq"] == st["seq"] and info["nst"] == len(ref)


def test_nested_packets(built):
    """A packet whose sub-channel data contain a complete valid AF packet: intact it is stepped over by its LEN, with the
    outer CRC broken the inner one is found -- a row in discovery, another plan's packet under the outer's plan."""
    intact, broken, inner = nested_pair()
    before, _ = make_packets("one_eep_a", 2, 5, start=698, seq=48)
    data = before[0] + before[1] + intact + broken + inner
    for streams in (CONFIGS["one_eep_a"](), None):
        case = Case(streams, data)
        got = run_host([case])[0]
        rows, result, _ = assert_is_reference(case, got)
        outer = [P.read_packet(x)["dlfc"] for x in (before[0], before[1], intact)]
        if streams is None:
            assert [r["status"]["dlfc"] for r in rows] == outer + [P.read_packet(inner)["dlfc"]] * 2
            assert rows[3]["status"]["offset"] == 3 * len(intact) + 136 + 11 + 20
        else:
            assert [r["status"]["dlfc"] for r in rows] == outer and result["other_plan"] == 2
        assert result["resyncs"] == 2                          # to the inner packet, and from its end to the next
        assert result["skipped"] == 136 + 11 + 20 + (len(intact) - 140 - (136 + 11 + 20))


def big_packet(total, seq, dlfc=5):
    """A FIC-only DETI packet of exactly `total` bytes, made with a large *dmy item"""
    core = P.PTR_DETI + P.item("deti", P.deti_value(dlfc, 0xFF, bytes(96)))
    p = P.af_packet(core + P.item("*dmy", bytes(total - 12 - len(core) - 8)), seq)
    assert len(p) == total
    return p


def test_size_seams(built):
    """Totals of exactly 8192 bytes (taken) and 8193 (not a candidate: its header is not plausible)."""
    small, _ = make_packets("fic_only", 2, 7, start=6, seq=2)
    data = big_packet(8192, 1) + small[0] + _too_big(8193, 3) + small[1]
    case = Case(None, data)
    got = run_host([case])[0]
    rows, result, _ = assert_is_reference(case, got)
    assert [(r["status"]["length"], r["status"]["dlfc"]) for r in rows] == [(8192, 5)] + [(140, P.read_packet(x)["dlfc"]) for x in small]
    assert result["skipped"] == 8193 and result["resyncs"] == 1
    assert [r["status"]["seq"] for r in rows] == [1, 2, 3] and not any(r["status"]["flags"] & RR.SEQ_BREAK for r in rows)


def _too_big(total, seq):
    core = P.PTR_DETI + P.item("deti", P.deti_value(5, 0xFF, bytes(96)))
    payload = core + P.item("*dmy", bytes(total - 12 - len(core) - 8))
    body = b"AF" + len(payload).to_bytes(4, "big") + seq.to_bytes(2, "big") + b"\x90T" + payload
    return body + synth.crc16(body).to_bytes(2, "big")


def _without_offsets(status):
    st = status.copy()
    st["offset"] = 0
    return st.tobytes()


def pieces_equal_whole(streams, data, cuts):
    """the stream fed in pieces cut at `cuts` leaves what one call leaves: rows, status (but the offsets, which count from the
    start of each call's S), the final state with its totals"""
    whole = run_host([Case(streams, data)])[0]
    n = int(whole["result"]["rows"])
    state, parts = None, []
    for a, b in zip([0] + list(cuts), list(cuts) + [len(data)]):
        got = run_host([Case(streams, data[a:b], state=state)])[0]
        state = got["state"]
        parts.append(got)
    rows = [int(g["result"]["rows"]) for g in parts]
    assert sum(rows) == n, (cuts, rows, n)
    assert _without_offsets(np.concatenate([g["status"][:k] for g, k in zip(parts, rows)])) == _without_offsets(whole["status"][:n]), cuts
    assert np.concatenate([g["fib"][:k] for g, k in zip(parts, rows)]).tobytes() == whole["fib"][:n].tobytes(), cuts
    assert np.concatenate([g["crc_ok"][:k] for g, k in zip(parts, rows)]).tobytes() == whole["crc_ok"][:n].tobytes(), cuts
    for i in range(len(whole["outs"])):
        assert np.concatenate([g["outs"][i][:k] for g, k in zip(parts, rows)]).tobytes() == whole["outs"][i][:n].tobytes(), cuts
    assert state.tobytes() == whole["state"].tobytes(), cuts
    return parts


def test_cut_at_every_byte_of_three_packets(built):
    pk, _ = make_packets("one_eep_a", 3, 9, start=4998, seq=65534)
    data = b"".join(pk)
    streams = CONFIGS["one_eep_a"]()
    for cut in range(len(data) + 1):
        pieces_equal_whole(streams, data, [cut])


def test_random_cuts_and_many_pieces_of_damaged_streams(built, damaged):
    rng = np.random.default_rng(11)
    for name in ("uep_and_eep_b", "tiny", "fic_only"):
        data, _ = damaged[name]
        streams = CONFIGS[name]()
        for _ in range(6):
            pieces_equal_whole(streams, data, [int(rng.integers(0, len(data) + 1))])
        cuts = sorted(int(x) for x in rng.integers(0, len(data) + 1, 40))
        parts = pieces_equal_whole(streams, data, cuts)
        # the reference agrees piece by piece (state records in, state records out)
        state = None
        for a, b, got in zip([0] + cuts, cuts + [len(data)], parts):
            case = Case(streams, data[a:b], state=state)
            assert_is_reference(case, got, what=(name, a, b))
            state = got["state"]
    pieces_equal_whole(None, damaged["uep_and_eep_b"][0], [1, 2, 3, 9, 10, 11, 12, 500, 501])


def test_discovery_and_unwanted_streams(built, damaged):
    data, ref = damaged["uep_and_eep_b"]
    streams = CONFIGS["uep_and_eep_b"]()
    none, some = Case(None, data), Case(streams, data, wanted=[True, False, True])
    a, b = run_host([none, some])
    rows, result, _ = assert_is_reference(none, a)
    assert_is_reference(some, b)
    assert result["other_plan"] == 0 and result["rows"] > int(b["result"]["rows"])
    # the multiplex is read from a row's packet, which its status locates
    st = a["status"][0]
    found = dabgpu.edi_streams(data[int(st["offset"]):int(st["offset"]) + int(st["length"])])
    assert sorted((s.subchannel_id, s.sc.start_address, s.sc.bitrate_kbps) for s in found) == \
        sorted((i, sc.start_address, sc.bitrate_kbps) for i, sc in streams)


@pytest.mark.parametrize("n", [0, 1, 9, 10, 11])
def test_short_inputs(built, n):
    pk, _ = make_packets("fic_only", 2, 13, start=3, seq=3)
    data = b"".join(pk)
    first = Case(None, data[:n])
    got = run_host([first])[0]
    _, result, new = assert_is_reference(first, got)
    assert result["rows"] == 0 and result["tail_bytes"] == n and result["skipped"] == 0
    second = Case(None, data[n:], state=got["state"])
    rows, result, _ = assert_is_reference(second, run_host([second])[0])
    assert [r["status"]["dlfc"] for r in rows] == [P.read_packet(x)["dlfc"] for x in pk] and result["skipped"] == 0 and result["resyncs"] == 0
    # garbage of that length: all but the last 9 bytes are given up
    junk = Case(None, bytes(range(1, n + 1)))
    _, result, _ = assert_is_reference(junk, run_host([junk])[0])
    assert result["tail_bytes"] == min(n, 9) and result["skipped"] == max(n - 9, 0)


def test_hostile_state_record_is_clamped(built):
    pk, _ = make_packets("fic_only", 2, 15, start=10, seq=0)
    rng = np.random.default_rng(16)
    state = rng.integers(0, 256, STATE_BYTES, dtype=np.uint8)
    head = state[:HEAD].view(dabgpu.EDI_READ_HEAD_DTYPE)
    head["tail_bytes"] = 0xFFFFFFF0
    head["last_dlfc"] = 60000
    head["have_prev"] = 1
    state[HEAD:HEAD + 8191] = 0x11                              # no "AF" in what counts as the tail
    case = Case(None, b"".join(pk), state=state)
    got = run_host([case])[0]
    rows, result, _ = assert_is_reference(case, got)
    assert result["rows"] == 2 and result["skipped"] == 8191 and rows[0]["status"]["gap"] == (rows[0]["status"]["dlfc"] - 60000 % 5000 - 1) % 5000


def test_refused_calls_write_nothing(built):
    pk, _ = make_packets("one_eep_a", 2, 17)
    streams = CONFIGS["one_eep_a"]()

    def refused(mutate):
        case = Case(streams, b"".join(pk))
        entries, keep = host_entries([case])
        mutate(entries[0], case)
        with pytest.raises(dabgpu.DabGpuError) as e:
            dabgpu.edi_read_host(entries)
        a = case.arrays
        assert all((x == FILL).all() for x in [a["state_out"], a["fib"], a["crc_ok"], a["status"], a["result"]] + a["outs"])
        return e.value.status == -1

    def bad_plan(e, c):
        c.plan.bytes[0] = 200

    def bad_stc(e, c):
        c.plan.header[11] ^= 1
    assert refused(lambda e, c: setattr(e, "n_bytes", -1))
    assert refused(lambda e, c: setattr(e, "d_bytes", e.d_bytes + 1))
    assert refused(lambda e, c: setattr(e, "d_state_out", None))
    assert refused(lambda e, c: setattr(e, "d_state_out", e.d_state_out + 8))
    assert refused(lambda e, c: setattr(e, "d_fib", None))
    assert refused(lambda e, c: setattr(e, "d_status", e.d_status + 4))
    assert refused(lambda e, c: setattr(e, "d_result", e.d_result + 2))
    assert refused(lambda e, c: setattr(e, "d_state_in", e.d_state_out + 16))
    assert refused(bad_plan) and refused(bad_stc)
    # a second entry's fault refuses the first too
    good, bad = Case(streams, pk[0]), Case(streams, pk[1])
    entries, keep = host_entries([good, bad])
    entries[1].d_result = None
    with pytest.raises(dabgpu.DabGpuError):
        dabgpu.edi_read_host(entries)
    assert (good.arrays["result"] == FILL).all() and (good.arrays["state_out"] == FILL).all()
    assert dabgpu.lib().dabgpu_edi_read_host(None, 1) == -1 and dabgpu.lib().dabgpu_edi_read_host(None, 0) == 0


def test_fuzz_program_under_sanitizers(built, tmp_path):
    """tests/edi_read_fuzz.cpp: the header alone, under AddressSanitizer and UBSan, on random and mutated streams and states,
    one of them header-plausible every 10 bytes."""
    exe = tmp_path / "edi_read_fuzz"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "edi_read_fuzz.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), "300"], text=True)
    assert "edi_read_fuzz ok" in out, out


def test_reader_kernels_use_no_scratch_and_spill_nothing(built, tmp_path):
    """The method of test_eti_read.py on the new code object: no scratch, no spills, no accumulation registers.  The walk
    kernel holds one packet (8 KB) and its fields record in LDS per single-wave workgroup: 160 KB / 9 KB lets 16 of them share
    a CU, four waves per SIMD, which at most 128 VGPRs a lane admit."""
    from test_device_asm import kernel_metadata
    csrc = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "csrc")
    obj, tools = os.path.join(csrc, "edi_read_kernels.o"), "/opt/rocm/lib/llvm/bin/"
    if not os.path.exists(obj):
        subprocess.check_call(["make", "-C", csrc, "edi_read_kernels.o"], stdout=subprocess.DEVNULL)
    fat, co = str(tmp_path / "edi_read.fat"), str(tmp_path / "edi_read.co")
    subprocess.check_call([tools + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([tools + "clang-offload-bundler", "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    md = kernel_metadata(subprocess.check_output([tools + "llvm-readelf", "--notes", co], text=True))
    assert sorted(k.split("edi_read_")[1].split("_kernel")[0] for k in md) == ["check", "walk"], list(md)
    for k, v in md.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v.get("agpr_count", 0) == 0 and v["vgpr_count"] <= 128, (k, v)
    walk = [v for k, v in md.items() if "edi_read_walk_kernel" in k][0]
    assert walk["group_segment_fixed_size"] <= 160 * 1024 // 16
    check = [v for k, v in md.items() if "edi_read_check_kernel" in k][0]
    assert check["vgpr_count"] <= 64 and check["group_segment_fixed_size"] <= 1024          # 8 waves per SIMD


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def rctx(built):
    from conftest import make_ctx
    c = make_ctx(None, max_frames=64)
    yield c
    c.close()


def run_dev(ctx, cases):
    import torch
    keep, entries = [], []
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    full = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    for c in cases:
        c.arrays = {"bytes": dev(np.frombuffer(c.data or b"\0", np.uint8).copy()), "state_in": None if c.state is None else dev(c.state),
                    "state_out": full(STATE_BYTES), "fib": full(c.rows * 96), "crc_ok": full(c.rows * 3), "status": full(c.rows * 32),
                    "result": full(48), "outs": [full(c.rows * n) for n in c.sizes]}
        entries.append(_entry(c, lambda x: x.data_ptr(), keep))
    ctx.edi_read_dev(entries)
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


def assert_device_is_host(ctx, make_cases, what=""):
    host_cases, dev_cases = make_cases(), make_cases()
    want, got = run_host(host_cases), run_dev(ctx, dev_cases)
    for i, (w, g) in enumerate(zip(want, got)):
        assert_same(g, w, "%s entry %d" % (what, i))
    return want


@pytest.mark.gpu
def test_device_all_plans_in_one_call_with_damage(rctx, damaged):
    want = assert_device_is_host(rctx, lambda: [Case(CONFIGS[n](), damaged[n][0]) for n in CONFIGS])
    for w in want:
        assert int(w["result"]["resyncs"]) >= 5 and int(w["result"]["other_plan"]) >= 1 and int(w["result"]["bad_tags"]) >= 1


@pytest.mark.gpu
def test_device_nested_packets(rctx):
    intact, broken, inner = nested_pair()
    before, _ = make_packets("one_eep_a", 2, 5, start=698, seq=48)
    data = before[0] + before[1] + intact + broken + inner
    want = assert_device_is_host(rctx, lambda: [Case(CONFIGS["one_eep_a"](), data), Case(None, data)])
    assert [int(w["result"]["rows"]) for w in want] == [3, 5]


@pytest.mark.gpu
def test_device_streams_that_start_inside_a_packet(rctx):
    pk, _ = make_packets("uep_and_eep_b", 6, 41, start=100, seq=1)
    data, n = b"".join(pk), len(pk[0])
    offsets = [0, 1, 2, 9, 10, 15, 16, n - 1]
    want = assert_device_is_host(rctx, lambda: [Case(CONFIGS["uep_and_eep_b"](), data[o:]) for o in offsets])
    assert [int(w["result"]["rows"]) for w in want] == [6] + [5] * 7
    assert [int(w["result"]["skipped"]) for w in want] == [0] + [n - o for o in offsets[1:]]


@pytest.mark.gpu
def test_device_130_packets_of_one_entry(rctx):
    """more than one 64-wide step of the search for the next good position: about 18 KB, and a damaged stretch far into the bitmap"""
    pk, _ = make_packets("fic_only", 130, 31, start=4900, seq=65500)
    data = b"".join(pk)
    assert len(data) == 130 * 140
    data = data[:100 * 140 + 77] + data[100 * 140 + 99:]
    data = data[:3 * 140] + bytes(64 * 70) + data[3 * 140:]      # 70 bitmap words without a packet
    want = assert_device_is_host(rctx, lambda: [Case(None, data), Case(CONFIGS["fic_only"](), data)])
    assert int(want[0]["result"]["rows"]) == 129 and int(want[0]["result"]["resyncs"]) == 2


@pytest.mark.gpu
def test_device_lengths_around_the_check_span(rctx):
    """stream lengths one below, at and one above the span of a workgroup of the check launch (4096 positions) and of one of its
    waves (64), with a packet straddling the seam; and the same with a carried tail in front"""
    pk, _ = make_packets("one_eep_a", 16, 43, start=20, seq=20)
    data = b"".join(pk)
    assert len(pk[0]) * 11 < 4096 - 64 and 4096 + 65 < len(pk[0]) * 12
    lengths = [4095, 4096, 4097, 4096 + 63, 4096 + 64, 4096 + 65, len(pk[0]) * 12 - 1, len(pk[0]) * 12]
    first = assert_device_is_host(rctx, lambda: [Case(CONFIGS["one_eep_a"](), data[:n]) for n in lengths], "first")
    assert [int(w["result"]["rows"]) for w in first] == [11] * 7 + [12]
    assert_device_is_host(rctx, lambda: [Case(CONFIGS["one_eep_a"](), data[n:], state=f["state"]) for n, f in zip(lengths, first)], "second")


def crc_chunk_flips(packet):
    """64 copies of the packet, copy i with a bit flipped in chunk i of the 64 its CRC is folded in (zero bytes in front up to
    64 equal chunks; a chunk that is all padding gives a flip in the first byte behind the header instead)"""
    L = len(packet) - 2
    cb = (L + 63) // 64
    lead = 64 * cb - L
    return [flip(packet, max(i * cb - lead + (cb - 1), 10), i % 8) for i in range(64)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["full_cif", "fic_only"])
def test_device_sees_a_flip_in_each_of_the_64_crc_chunks(rctx, name):
    pk, _ = make_packets(name, 2, 5, start=50, seq=50)
    data = b"".join(crc_chunk_flips(pk[1])) + pk[0]
    want = assert_device_is_host(rctx, lambda: [Case(CONFIGS[name](), data), Case(None, data)])
    for w in want:
        assert int(w["result"]["rows"]) == 1 and int(w["result"]["resyncs"]) == 1 and int(w["result"]["skipped"]) == 64 * len(pk[0])


@pytest.mark.gpu
def test_device_size_seams(rctx):
    small, _ = make_packets("fic_only", 2, 7, start=6, seq=2)
    data = big_packet(8192, 1) + small[0] + _too_big(8193, 3) + small[1]
    want = assert_device_is_host(rctx, lambda: [Case(None, data), Case(None, data[:8191]), Case(None, data[:8192])])
    assert [int(w["result"]["rows"]) for w in want] == [3, 0, 1] and int(want[1]["result"]["tail_bytes"]) == 8191


@pytest.mark.gpu
def test_device_unwanted_streams_and_discovery(rctx, damaged):
    data = damaged["multiplex18"][0]
    wanted = [k % 3 != 1 for k in range(18)]
    assert_device_is_host(rctx, lambda: [Case(CONFIGS["multiplex18"](), data, wanted=wanted), Case(None, data),
                                         Case(CONFIGS["multiplex18"](), data, wanted=[False] * 18), Case(CONFIGS["tiny"](), b""),
                                         Case(None, data[:9]), Case(None, data[:10]), Case(None, data[:11])])


@pytest.mark.gpu
def test_device_two_calls_with_the_carry_equal_the_host_calls(rctx, damaged):
    names = ["uep_and_eep_b", "full_cif", "tiny"]
    cuts = {"uep_and_eep_b": 9 * 348 + 301, "full_cif": 8191, "tiny": 17 * 180 + 5}
    first = assert_device_is_host(rctx, lambda: [Case(CONFIGS[n](), damaged[n][0][:cuts[n]]) for n in names], "first")
    hostile = np.full(STATE_BYTES, 0xFF, np.uint8)
    assert_device_is_host(rctx, lambda: [Case(CONFIGS[n](), damaged[n][0][cuts[n]:], state=f["state"]) for n, f in zip(names, first)] +
                          [Case(CONFIGS["tiny"](), damaged["tiny"][0][:3000], state=hostile)], "second")


@pytest.mark.gpu
def test_device_refused_calls_write_nothing(rctx):
    import torch
    pk, _ = make_packets("tiny", 2, 11)
    case = Case(CONFIGS["tiny"](), b"".join(pk), state=np.zeros(STATE_BYTES, np.uint8))
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
                entry(d_fib=addr(a["fib"]) + 4), entry(d_state_in=addr(a["state_in"]) + 8), entry(d_status=None)):
        with pytest.raises(dabgpu.DabGpuError) as e:
            rctx.edi_read_dev([entry(), bad])
        assert e.value.status == -1
    rctx.sync()
    for k in ("fib", "crc_ok", "status", "result", "state_out"):
        assert bool((a[k] == FILL).all()), k
    assert bool((a["outs"][0] == FILL).all())


@pytest.mark.gpu
def test_round_trip_and_the_follow_call_on_the_readers_rows(rctx):
    """Decode buffers -> dabgpu_edi_frames_dev -> dabgpu_edi_read_dev: the same sub-channel rows, the FIBs 15 CIFs late as
    documented with the CRC flags the bytes really have, the whole count and the sequence numbers; and
    dabgpu_dabplus_follow_dev finds on the reader's rows the access units it finds on the buffers that went into the writer."""
    import torch
    from test_edi import run_edi
    from test_eti import SERVICES
    ens = synth.ServiceEnsemble(7, SERVICES[:1], n_frames=10, extras=False)
    streams = [(3, dabgpu.subchannel(0, 64, level=3))]
    n_cif = 40
    lf = np.ascontiguousarray(np.asarray(ens.msc_bytes[0], np.uint8)[:n_cif]).reshape(1, n_cif, 192)
    fib, ok = make_fibs(np.random.default_rng(1), n_cif)
    claimed = ok.copy()
    claimed[20] ^= 1                                          # flags that do not say what the bytes say
    edi, _, _, packet = run_edi(rctx, streams, fib[None], claimed[None], [lf], cif_start=[4990], seq_start=[65530], slack=0)
    stream = np.ascontiguousarray(edi[:, :n_cif * packet])
    got_fib, got_ok, outs, status, result, _ = rctx.edi_read(torch.from_numpy(stream).cuda(), streams)
    res = result.cpu().numpy().view(dabgpu.EDI_READ_RESULT_DTYPE).reshape(-1)[0]
    assert int(res["rows"]) == n_cif and not res["skipped"] and not res["tail_bytes"] and not res["gap_sum"] and not res["resyncs"]
    assert outs[0].cpu().numpy()[0, :n_cif].tobytes() == lf.tobytes()
    got_fib, got_ok = got_fib.cpu().numpy()[0], got_ok.cpu().numpy()[0]
    assert not got_fib[:15].any() and got_fib[15:n_cif].tobytes() == fib[:n_cif - 15].tobytes()
    assert got_ok[15:n_cif].tobytes() == ok[:n_cif - 15].tobytes()
    st = status.cpu().numpy().view(dabgpu.EDI_READ_STATUS_DTYPE).reshape(-1)[:n_cif]
    assert list(st["dlfc"]) == [(4990 - 15 + t) % 5000 for t in range(n_cif)] and list(st["seq"]) == [(65530 + t) % 65536 for t in range(n_cif)]
    assert not (st["flags"] & (dabgpu.EDI_READ_GAP | dabgpu.EDI_READ_SEQ_BREAK | dabgpu.EDI_READ_FP_MISMATCH | dabgpu.EDI_READ_NO_FIC)).any()
    assert (st["flags"][:15] & dabgpu.EDI_READ_STAT_FIELD).all() and (st["stat"][:15] == 0).all()

    def follow(d_in):
        z = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")
        carry, data, status, res = z(dabgpu.dabplus_carry_bytes(64)), z(8 * 110 * 8), z(8 * 64), z(32)
        rctx.dabplus_follow_dev([dabgpu.DabplusEntry(d_in.data_ptr(), 192, 64, None, carry.data_ptr(), data.data_ptr(), status.data_ptr(),
                                                     res.data_ptr())], n_cif)
        rctx.sync()
        return data.cpu().numpy(), status.cpu().numpy(), res.cpu().numpy().view(dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)[0], carry.cpu().numpy()
    a = follow(torch.from_numpy(lf.reshape(n_cif, 192)).cuda())
    b = follow(outs[0][0, :n_cif].contiguous())
    assert int(a[2]["n_superframes"]) >= 1 and a[2].tobytes() == b[2].tobytes()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes()


# ------------------------------------------------------------------ the host mirror
HOST = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "host")


import functools


@functools.lru_cache(maxsize=None)
def mirror_stream():
    """Three cycles of the synthetic ensemble of the ETI mirror test -- a DAB+ service with a dynamic label, a layer-II service,
    a packet-mode component -- as AF packets from the reference writer with a *dmy packet between every two
    -> (ens, the packets, the *dmy packet, the stream)"""
    import test_mp2_end_to_end as E
    import test_packet as PK
    _pe, frames = PK.e2e_ensemble()
    service = ("Slides", 0xD301, PK.E2E_SUBCH, 0, 3, 32, PK.E2E_START, [(PK.E2E_SCID, PK.ADDR, synth.DSCTY_MOT, 0)], frames, 0)
    bodies, _plain = E.dabplus_bodies()
    ens = synth.ServiceEnsemble(E.SEED, E.SERVICES, n_frames=5, dab_services=E.DAB, extras=False, bodies=bodies, dab_pads=[E.mp2_pads()],
                                packet_services=[service])
    streams = [{"id": 3, "start": 0, "bitrate": 64, "uep": False, "eep_type": 0, "level": 3},
               {"id": PK.E2E_SUBCH, "start": PK.E2E_START, "bitrate": 32, "uep": False, "eep_type": 0, "level": 3},
               ref_stream(11, dabgpu.uep_subchannel(17, 100))]
    fibs = ens.fibs.reshape(20, 96)
    sent = {3: ens.msc_bytes[0], PK.E2E_SUBCH: frames, 11: ens.mp2_frames[0]}
    dmy = P.af_packet(P.item("*dmy", bytes(16)), 0)
    pk = [P.write_packet(streams, c, 2 * c, fibs[c % 20].tobytes(), {i: bytes(d[c % 20]) for i, d in sent.items()}, 0xFF) for c in range(60)]
    edi = b"".join(p + dmy for p in pk)
    n = len(pk[0]) + len(dmy)
    return ens, pk, dmy, edi


def test_mirror_reads_an_edi_stream_in_uneven_pieces(built, tmp_path):
    """tests/edi_read_mirror_check.cpp: BasicRadio::ProcessEdi over the TEST-ONLY fake ABI (unchanged: the walk is the header's,
    no new symbol).  Three cycles of the synthetic ensemble of the ETI mirror test -- a DAB+ service with a dynamic label, a
    layer-II service, a packet-mode component -- as AF packets from the reference writer with a *dmy packet between every two,
    fed in uneven pieces: the services, the label and the counts ProcessEti gives on the same ensemble as ETI(NI)."""
    import test_mp2_end_to_end as E
    import test_packet as PK
    fake, oracle = os.path.join(ROOT, "tests", "fake_abi"), os.path.join(ROOT, "oracle")
    assert "edi" not in open(os.path.join(fake, "fake_dabgpu.cpp")).read()
    exe = str(tmp_path / "edi_read_mirror_check")
    srcs = [os.path.join(ROOT, "tests", "edi_read_mirror_check.cpp"), os.path.join(fake, "fake_dabgpu.cpp")]
    srcs += [os.path.join(HOST, s) for s in ("ofdm/ofdm_demodulator.cpp", "basic_radio/basic_radio.cpp", "basic_radio/basic_dab_plus_channel.cpp", "dab/fic/fic_parser.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), "-I" + oracle, "-I" + fake] + srcs +
                          ["-L" + oracle, "-loracle", "-Wl,-rpath," + oracle, "-o", exe])
    ens, pk, dmy, edi = mirror_stream()
    n = len(pk[0]) + len(dmy)
    cut = edi[:45 * n + 100] + edi[45 * n + 200:]                              # ... and once more with 100 bytes lost in packet 45

    def run(data, pieces):
        path = tmp_path / "in.edi"
        path.write_bytes(data)
        r = subprocess.run([exe, str(path)] + [str(p) for p in pieces], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return {l.split()[0] + (" " + l.split()[1] if l.split()[0] in ("channel", "packet", "service") else ""): dict(kv.split("=", 1) for kv in l.split()[1:])
                for l in r.stdout.splitlines()}
    out = run(edi, [1, 500, n - 1, 17, 20000, n + 1])
    read = {k: int(v) for k, v in out["read"].items()}
    assert (read["rows"], read["not_deti"], read["bad_tags"], read["skipped"], read["resyncs"], read["gap_sum"], read["fib_errors"], read["tail"],
            read["fibs"]) == (60, 60, 0, 0, 0, 0, 0, 0, 180), read
    assert bytes.fromhex(out["ensemble"]["label"]).rstrip() == b"Synth Ensemble"
    assert sorted(bytes.fromhex(out[k]["label"]).rstrip() for k in out if k.startswith("service")) == [b"Classic", b"Radio One", b"Slides"]
    plus, mp2, packet = out["channel subchannel=3"], out["channel subchannel=11"], out["packet subchannel=%d" % PK.E2E_SUBCH]
    per_sf = [len(a) for a in ens.aus[0]]                                      # access units per super-frame of the cycle
    assert int(plus["superframes"]) == 11 and int(plus["aus"]) == int(plus["handed"]) == 3 * sum(per_sf) - per_sf[0] and plus["au_errors"] == "0"
    assert bytes.fromhex(plus["label"]) == E.LABELS[0]
    assert (int(mp2["mp2_frames"]), int(mp2["handed"]), mp2["header_errors"], mp2["crc_errors"]) == (59, 59, "0", "0")
    assert bytes.fromhex(mp2["label"]) == E.LABELS[1]
    assert (int(packet["frames"]), packet["addresses"], packet["objects"]) == (59, "1", "1")
    out = run(cut, [701, 3])
    read = {k: int(v) for k, v in out["read"].items()}
    assert (read["rows"], read["not_deti"], read["skipped"], read["resyncs"], read["gap_sum"], read["tail"]) == (59, 60, len(pk[0]) - 100, 1, 1, 0), read
    assert int(out["channel subchannel=11"]["mp2_frames"]) == 58


def test_edi_play_lists_the_services_on_the_host(built, tmp_path):
    """tools/edi_play.py --host (no GPU: edi_read_host, then the FIG oracle) on the mirror test's stream with a damaged stretch
    and a foreign packet in it: the multiplex, the ensemble and the three services tools/eti_play.py lists from the same FIBs, and
    the reader's counters."""
    import sys
    ens, pk, dmy, edi = mirror_stream()
    n = len(pk[0]) + len(dmy)
    path = tmp_path / "in.edi"
    path.write_bytes(edi[200:45 * n + 100] + edi[45 * n + 200:])              # begins inside a packet, 100 bytes lost in packet 45
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "edi_play.py"), "--host", "--chunk-bytes", "5000", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("multiplex of the packet at byte %d (dlfc 1, SEQ 2): 3 streams" % (n - 200))
    assert "(3, 0, 64)" in lines[0] and "(11, 100, 64)" in lines[0]
    from oracle import fig_oracle as FO
    want = [l for l in FO.parse_fibs(ens.fibs.reshape(-1, 32)).lines() if l.split()[0] in ("ensemble", "service", "subchannel", "component")]
    assert lines[1:-1] == want and sum(l.startswith("service ") for l in want) == 3
    read = dict(kv.split("=") for kv in lines[-1].split()[1:])
    assert (read["rows"], read["not_deti"], read["bad_tags"], read["other_plan"], read["resyncs"], read["gap_sum"], read["tail_bytes"]) == \
        ("58", "60", "0", "0", "2", "1", "0"), read            # (every *dmy packet is whole)
    assert int(read["skipped"]) == (len(pk[0]) - 200) + (len(pk[0]) - 100)      # (the *dmy packet behind either stretch is whole)
