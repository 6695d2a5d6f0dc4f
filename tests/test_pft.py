"""EDI PFT layer (include/dabgpu.h, "EDI PFT layer"; include/dabgpu_pft.h): AF packets cut into PF fragments with RS(255,207)
and PF fragment byte streams put back together.  The host calls are held byte for byte to tests/pft_reference.py (the contract
in plain Python: parity by polynomial division, erasures by Gaussian elimination) -- fragments, records, output, result and
state; the device calls byte for byte to the host calls.  Outputs start out as 0xEE so that what a call must not write is
compared too."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
import pft_reference as R
from conftest import ROOT
from test_eti_read import aligned

FILL = 0xEE
STATE_BYTES = R.STATE_BYTES
REC, RES = dabgpu.PFT_READ_RECORD_DTYPE, dabgpu.PFT_READ_RESULT_DTYPE
SIZES = [12, 140, 207, 208, 414, 415, 8192]        # c = 1 | c = 2, z = 0, k = 104 and 207 | c = 3, z = 2 | c = 40


# ------------------------------------------------------------------ packets, fragments, damage
def make_af(l, seed, seq=0):
    """a valid AF packet of l bytes with a random payload"""
    body = np.random.default_rng(seed).integers(0, 256, l - 12, dtype=np.uint8).tobytes()
    p = b"AF" + (l - 12).to_bytes(4, "big") + (seq & 0xFFFF).to_bytes(2, "big") + b"\x90T" + body
    return p + R.crc16(p).to_bytes(2, "big")


def lib_layout(a):
    return dabgpu.pft_layout(a["packet_bytes"], a["fec"], a["m"], a["max_payload"], a["addr"])


def frags_of(l, seed, pseq, m=2, fec=True, addr=False, max_payload=1400):
    """(AF packet, its fragments from the reference writer, the layout dict)"""
    a = R.layout(l, fec, m, max_payload, addr)
    af = make_af(l, seed, pseq)
    return af, R.fragments(af, a, pseq, 0x1234, 0xABCD), a


def custom_frags(af, c, k, f, s, pseq, drop=()):
    """fragments of a layout the writer's rule would not choose (the reader takes any consistent one)"""
    a = dict(fec=1, addr=0, chunks=c, rs_k=k, rs_z=c * k - len(af), block_bytes=c * (k + 48), fcount=f, plen=s)
    assert f * s >= a["block_bytes"] and f * s // (k + 48) == c and a["rs_z"] >= 0
    return [x for g, x in enumerate(R.fragments(af, a, pseq)) if g not in set(drop)]


def flip(data, pos, bit=0):
    b = bytearray(data)
    b[pos] ^= 1 << bit
    return bytes(b)


def worst_erasures(a, dropped):
    return int(R.chunk_counts(a["chunks"], a["rs_k"], a["fcount"])[:, sorted(dropped)].sum(1).max()) if dropped else 0


def drop_set_with(a, want):
    """a set of fragments whose loss leaves exactly `want` erasures in the worst chunk"""
    counts = R.chunk_counts(a["chunks"], a["rs_k"], a["fcount"])
    rng = np.random.default_rng(want)
    for _ in range(200):
        order, picked = rng.permutation(a["fcount"]), []
        for g in order:
            if counts[:, picked + [int(g)]].sum(1).max() <= want:
                picked.append(int(g))
            if counts[:, picked].sum(1).max() == want:
                return picked
    return None                                                                   # (this layout's sums pass over it)


# ------------------------------------------------------------------ running the calls
class Case:
    """One entry: the new bytes, the state record (uint8 [STATE_BYTES]) or None, FLUSH."""

    def __init__(self, data, state=None, flush=False):
        self.data, self.state, self.flush = bytes(data), state, flush
        self.n_out, self.n_rec = dabgpu.pft_read_out_bytes(len(self.data)), dabgpu.pft_read_max_records(len(self.data))


def _entry(c, addr):
    a = c.arrays
    return dabgpu.PftReadEntry(addr(a["bytes"]) if len(c.data) else None, len(c.data), dabgpu.PFT_READ_FLUSH if c.flush else 0,
                               None if a["state_in"] is None else addr(a["state_in"]), addr(a["state_out"]), addr(a["out"]), addr(a["records"]),
                               addr(a["result"]))


def _collect(c, get):
    a = c.arrays
    return {"out": get(a["out"]), "records": get(a["records"]).view(REC).reshape(-1), "result": get(a["result"]).view(RES)[0],
            "state": get(a["state_out"])}


def host_entries(cases):
    for c in cases:
        c.arrays = {"bytes": aligned(max(len(c.data), 1)), "state_in": None, "state_out": aligned(STATE_BYTES), "out": aligned(c.n_out),
                    "records": aligned(c.n_rec * 32), "result": aligned(64)}
        c.arrays["bytes"][:len(c.data)] = np.frombuffer(c.data, np.uint8)
        if c.state is not None:
            c.arrays["state_in"] = aligned(STATE_BYTES)
            c.arrays["state_in"][:] = c.state
    return [_entry(c, lambda x: x.ctypes.data) for c in cases]


def run_host(cases):
    dabgpu.pft_read_host(host_entries(cases))
    return [_collect(c, lambda x: x.copy()) for c in cases]


def ref_records(records):
    out = np.zeros(len(records), REC)
    for i, r in enumerate(records):
        for k, v in r.items():
            out[i][k] = v
    return out


def assert_is_reference(got, ref, what=""):
    """one result of _collect against one result of R.read, byte for byte, the untouched bytes included"""
    records, out, result, state = ref
    for k in RES.names:
        assert int(got["result"][k]) == result[k], "%s result.%s: %d, reference %d (%s)" % (what, k, got["result"][k], result[k], got["result"])
    n = len(records)
    assert got["records"][:n].tobytes() == ref_records(records).tobytes(), "%s records:\n%s\nreference\n%s" % (what, got["records"][:n], records)
    assert (got["records"][n:].view(np.uint8) == FILL).all(), what + " records behind the last are written"
    assert got["out"][:len(out)].tobytes() == out and (got["out"][len(out):] == FILL).all(), what + " output"
    want = R.pack_state(state)
    if got["state"].tobytes() != want.tobytes():
        bad = np.nonzero(got["state"] != want)[0]
        pytest.fail("%s state differs at bytes %s (%d in all)" % (what, bad[:8], bad.size))


def check_calls(pieces, flush_last=True, what=""):
    """a stream given in pieces: every call against the reference; -> (all records, all output, the last state) of the reference"""
    st, lib_state, all_records, all_out = R.new_state(), None, [], b""
    for i, piece in enumerate(pieces):
        flush = flush_last and i == len(pieces) - 1
        ref = R.read(st, piece, flush)
        got = run_host([Case(piece, lib_state, flush)])[0]
        assert_is_reference(got, ref, "%s call %d" % (what, i))
        st, lib_state = ref[3], got["state"]
        all_records += [dict(r, offset=r["offset"] + len(all_out)) for r in ref[0]]
        all_out += ref[1]
    return all_records, all_out, st


def flags_of(records):
    return [r["flags"] for r in records]


# ------------------------------------------------------------------ CPU: sizes, the format, the layout
def test_sizes_and_constants_are_the_headers(built):
    hdr = open(os.path.join(ROOT, "include", "dabgpu_pft.h")).read()
    const = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (\w+) = (\d+);", hdr)}
    assert const["FIRST_ROOT"] == R.FIRST_ROOT == 1 and const["PARITY"] == 48 and const["RS_K"] == 207 and const["MAX_CHUNKS"] == 40
    assert const["MAX_BLOCK"] == R.MAX_BLOCK == 10496 and const["MAX_PLEN"] == 8192 and const["MAX_FRAGMENTS"] == 256 and const["LATE_RUN"] == 16
    assert dabgpu.pft_read_state_bytes() == STATE_BYTES == 144 + 2 * (64 + 10496) + 8224 and STATE_BYTES % 16 == 0
    assert dabgpu.pft_read_out_bytes(0) == R.OUT_SLACK and dabgpu.pft_read_out_bytes(1000) == R.OUT_SLACK + 1000
    assert dabgpu.pft_read_max_records(0) == 2 + 8211 // 15 and dabgpu.pft_read_max_records(150) == 2 + 8361 // 15
    assert dabgpu.pft_read_out_bytes(-1) == 0 and dabgpu.pft_read_max_records((1 << 30) + 1) == 0
    import ctypes as C
    assert C.sizeof(dabgpu.PftLayout) == 64 and C.sizeof(dabgpu.PftReadEntry) == 56 and REC.itemsize == 32 and RES.itemsize == 64
    assert dabgpu.PFT_READ_HEAD_DTYPE.itemsize == 144 == R.HEAD_DTYPE.itemsize
    assert [dabgpu.PFT_FEC, dabgpu.PFT_ADDR, dabgpu.PFT_RECOVERED, dabgpu.PFT_INCONSISTENT, dabgpu.PFT_LOST, dabgpu.PFT_AF_OK,
            dabgpu.PFT_FLUSHED] == [R.FEC, R.ADDR, R.RECOVERED, R.INCONSISTENT, R.LOST, R.AF_OK, R.FLUSHED]
    abi = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    for name, value in (("FEC", 1), ("ADDR", 2), ("RECOVERED", 4), ("INCONSISTENT", 8), ("LOST", 16), ("AF_OK", 32), ("FLUSHED", 64), ("READ_FLUSH", 1)):
        assert re.search(r"#define DABGPU_PFT_%s\s+%d\b" % (name, value), abi), name
    for name in ("dabgpu_pft_layout", "dabgpu_pft_fragments_dev", "dabgpu_pft_read_dev", "dabgpu_pft_read_host"):
        assert name in dabgpu.EXPORTS and getattr(dabgpu.lib(), name).argtypes is not None


#: the three fragments of the 12-byte AF packet "AF" 00000000 0007 90 'T' + CRC with Pseq 0x0102, m = 1: c = 1, k = 12, z = 0,
#: B = 60, s0 = 24, f = 3, s = 20.  Header: "PF", Pseq, Findex, Fcount, 0x8000 | 20, RSk 12, RSz 0, HCRC; payload = block bytes
#: g, g + 3, g + 6, ... of the packet followed by its 48 parity bytes.
KNOWN_PACKET = bytes.fromhex("4146000000000007905481c2")
KNOWN_FRAGMENTS = [
    "504601020000000000038014" "0c00" "2484" "410000548fb5abb577bd316352c78eb8bb6b0f88",
    "504601020000010000038014" "0c00" "6357" "4600078127deeeb1c9aa338c92c8b40bf91b3b41",
    "504601020000020000038014" "0c00" "ab22" "000090c203cb253c8867610e8f369443d12379c9",
]


def test_known_answer_fragments(built):
    """l = 12, m = 1, written out: what pins the format (field order, HCRC, generator, interleave) for a reader of the test."""
    assert KNOWN_PACKET == b"AF\0\0\0\0\0\x07\x90T" + R.crc16(b"AF\0\0\0\0\0\x07\x90T").to_bytes(2, "big")
    a = R.layout(12, True, 1, 1400, False)
    assert (a["chunks"], a["rs_k"], a["rs_z"], a["block_bytes"], a["fcount"], a["plen"], a["guaranteed_losses"]) == (1, 12, 0, 60, 3, 20, 2)
    want = [bytes.fromhex(x) for x in KNOWN_FRAGMENTS]
    assert R.fragments(KNOWN_PACKET, a, 0x0102) == want
    got = dabgpu.pft_fragments_host(lib_layout(a), np.frombuffer(KNOWN_PACKET, np.uint8)[None], [0x0102])
    assert got.tobytes() == b"".join(want)
    block = KNOWN_PACKET + R.parity(KNOWN_PACKET)
    assert all(R.evaluate(block, e) == 0 for e in range(1, 49)) and R.evaluate(block, 49) != 0 and R.evaluate(block, 0) != 0
    # any two of the three may be lost
    for keep in range(3):
        recs, out, res, _ = R.read(R.new_state(), want[keep], True)
        assert out == KNOWN_PACKET and recs[0]["flags"] == R.FEC | R.RECOVERED | R.AF_OK | R.FLUSHED and recs[0]["max_erasures"] == 40


def _subset_masks(f):
    m = ((np.arange(1 << f)[:, None] >> np.arange(f)) & 1).astype(np.int64)
    return m, m.sum(1)


def test_layout_is_the_references_for_every_size(built):
    """Every l in 12 .. 8192 with m in {0, 1, 2, 3, 5, 8}: the fields, the refusals, guaranteed_losses >= m, and guaranteed_losses
    exact against brute force over all subsets of fragments where f <= 12."""
    masks = {}
    L = dabgpu.lib()
    info = dabgpu.PftLayout()
    import ctypes as C
    names = [n for n, _ in dabgpu.PftLayout._fields_ if n != "reserved"]
    brute = 0
    for m in (0, 1, 2, 3, 5, 8):
        for l in range(12, 8193):
            a = R.layout(l, True, m, 1400, False)
            rc = L.dabgpu_pft_layout(l, 1, m, 1400, 0, C.byref(info))
            assert (rc == 0) == (a is not None), (l, m)
            if a is None:
                continue
            assert {n: getattr(info, n) for n in names} == a, (l, m)
            assert a["guaranteed_losses"] >= m and a["fcount"] * a["plen"] // (a["rs_k"] + 48) == a["chunks"]
            f = a["fcount"]
            if f <= 12:
                if f not in masks:
                    masks[f] = _subset_masks(f)
                sub, size = masks[f]
                counts = np.unique(R.chunk_counts(a["chunks"], a["rs_k"], f), axis=0)        # (chunks that the fragments share alike count once)
                worst = (sub @ counts.T).max(1)                                             # per subset: its worst chunk
                ok_sizes = [n for n in range(f + 1) if (worst[size == n] <= 48).all()]
                g = max(n for n in ok_sizes if all(k in ok_sizes for k in range(n + 1)))
                assert g == a["guaranteed_losses"], (l, m, g, a)
                brute += 1
    assert brute > 16000                                                          # (every size at m = 0 and m = 1)
    # the issue's two examples, and the refusals
    a = R.layout(8192, True, 2)
    assert (a["chunks"], a["rs_k"], a["rs_z"], a["fcount"], a["guaranteed_losses"]) == (40, 205, 8, 16, 3)
    a = R.layout(415, True, 3)
    assert (a["chunks"], a["rs_k"], a["rs_z"], a["fcount"], a["guaranteed_losses"]) == (3, 139, 2, 16, 4)
    for args in ((11, 1, 2, 1400, 0), (8193, 1, 2, 1400, 0), (100, 1, -1, 1400, 0), (100, 1, 2, 0, 0), (8192, 0, 0, 31, 0), (8192, 1, 2, 30, 0),
                 (100, 1, 48, 1400, 0)):
        before = bytes(info)
        assert L.dabgpu_pft_layout(*args, C.byref(info)) == -1 and bytes(info) == before and R.layout(*args[:4], bool(args[4])) is None, args
    assert L.dabgpu_pft_layout(100, 1, 2, 1400, 0, None) == -1
    for l, s in ((12, 5), (100, 100), (8192, 32), (5000, 1400)):
        a = R.layout(l, False, 0, s, True)
        assert {n: getattr(dabgpu.pft_layout(l, False, 0, s, True), n) for n in names} == a and a["header_bytes"] == 18


@pytest.mark.parametrize("l", SIZES)
def test_host_writer_is_the_reference(built, l):
    for m, fec, addr in ((0, True, False), (2, True, True), (5, True, False), (0, False, False), (0, False, True)):
        a = R.layout(l, fec, m, 1400 if fec else 100, addr)
        if a is None:
            continue
        afs = [make_af(l, 100 * l + 7 * m + n, n) for n in range(3)]
        want = [b"".join(b"".join(R.fragments(af, a, (pseq0 + n) & 0xFFFF, 0x1234, 0xABCD)) for n, af in enumerate(afs)) for pseq0 in (65534, 9)]
        got = dabgpu.pft_fragments_host(lib_layout(a), np.frombuffer(b"".join(afs), np.uint8)[None].repeat(2, 0), [65534, 9], 0x1234, 0xABCD)
        assert [g.tobytes() for g in got] == want, (l, m, fec, addr)
        if fec:
            # every parity byte, by the definition: the codeword vanishes at alpha^1 .. alpha^48
            block = R.rs_block(afs[0], a)
            c, k = a["chunks"], a["rs_k"]
            for i in range(c):
                cw = block[i * k:(i + 1) * k] + block[c * k + 48 * i:c * k + 48 * (i + 1)]
                assert all(R.evaluate(cw, e) == 0 for e in range(1, 49)), (l, i)


def test_writer_refusals_write_nothing(built):
    import ctypes as C
    L = dabgpu.lib()
    lay = dabgpu.pft_layout(140, True, 2)
    src, dst = aligned(160), aligned(4096)
    call = lambda layout=lay, n_streams=1, n_packets=1, s=src, ins=160, source=0, d=dst, outs=4096: L.dabgpu_pft_fragments_host(
        C.byref(layout), n_streams, n_packets, s.ctypes.data, ins, None, source, 0, d.ctypes.data, outs)
    assert call() == 0 and not (dst[:lay.stream_bytes] == FILL).all()
    dst[:] = FILL
    bad = dabgpu.pft_layout(140, True, 2)
    bad.plen += 1
    for kw in (dict(layout=bad), dict(n_streams=-1), dict(n_packets=-1), dict(ins=100), dict(outs=16), dict(ins=161), dict(source=0x10000),
               dict(s=src[1:]), dict(d=dst[1:]), dict(d=src)):
        assert call(**kw) == -1, kw
    assert (dst == FILL).all()
    assert L.dabgpu_pft_fragments_host(None, 1, 1, src.ctypes.data, 160, None, 0, 0, dst.ctypes.data, 4096) == -1


# ------------------------------------------------------------------ CPU: the reader on the writer's fragments
@pytest.fixture(scope="module")
def loss_cases():
    """name -> (the stream, its AF packet, held to the Python reference?): every loss case of the reader, each a stream of its
    own.  The sets of guaranteed_losses fragments are exhaustive where C(f, n) <= 2000 (l = 8192, m = 2: all 560) and 200 seeded
    draws otherwise.  Of the 8192-byte packets' sets every ninth goes through the Python reference (its elimination takes a
    quarter of a second for 40 chunks); the others are held to the AF packet, the flags and the counters."""
    cases = {}
    for l in SIZES:
        for m in (0, 2):
            af, fr, a = frags_of(l, l + m, 40000 + l, m)
            f, g = a["fcount"], a["guaranteed_losses"]
            cases["whole l=%d m=%d" % (l, m)] = (b"".join(fr), af, True)
            for miss in range(f):
                cases["l=%d m=%d without %d" % (l, m, miss)] = (b"".join(x for i, x in enumerate(fr) if i != miss), af, True)
            subsets = list(itertools.combinations(range(f), g))
            if len(subsets) > 2000:
                rng = np.random.default_rng(l)
                subsets = [tuple(rng.choice(f, g, replace=False)) for _ in range(200)]
            for n, sub in enumerate(subsets):
                cases["l=%d m=%d without %s" % (l, m, sub)] = (b"".join(x for i, x in enumerate(fr) if i not in sub), af, l != 8192 or n % 9 == 0)
    return cases


def test_host_reader_recovers_every_guaranteed_loss(built, loss_cases):
    """None missing, every single fragment missing, any guaranteed_losses fragments missing (exhaustively where C(f, n) <= 2000,
    200 seeded draws otherwise): the packet comes back.  Every case is held to the AF packet, the record's flags and the
    counters; all of them but eight in nine of the 8192-byte packet's sets are held to the Python reference byte for byte as
    well (the fixture says why)."""
    assert sum("l=8192 m=2 without (" in name for name in loss_cases) == 560
    for name, (data, af, through_reference) in loss_cases.items():
        if through_reference:
            records, out, _ = check_calls([data], what=name)
            assert len(records) == 1 and out == af, name
    names = list(loss_cases)
    for at in range(0, len(names), 100):
        batch = names[at:at + 100]
        for name, got in zip(batch, run_host([Case(loss_cases[n][0], None, True) for n in batch])):
            af, res, rec = loss_cases[name][1], got["result"], got["records"][0]
            lost = "without" in name
            assert (res["records"], res["packets"], res["lost"], res["recovered"], res["out_bytes"]) == (1, 1, 0, int(lost), len(af)), (name, res)
            assert got["out"][:len(af)].tobytes() == af and (got["out"][len(af):] == FILL).all(), name
            assert rec["length"] == len(af) and rec["flags"] == R.FEC | R.AF_OK | R.FLUSHED * lost | R.RECOVERED * lost, (name, rec)
            assert (rec["max_erasures"] > 0) == lost and rec["max_erasures"] <= 48 and (res["chunks_filled"] > 0) == lost, (name, rec)


def test_host_reader_at_the_edge_of_the_code(built):
    """Exactly 48 erasures in the worst chunk: recovered; exactly 49: LOST.  The first and the last fragment missing, the
    latter with padding positions >= B.  A flipped payload byte in a group with erasures: INCONSISTENT, no AF_OK; in a
    complete group: emitted, no AF_OK."""
    hit = {48: 0, 49: 0}
    for l, m in ((8192, 2), (415, 8), (2476, 5), (1000, 3), (5896, 8), (300, 5)):
        af, fr, a = frags_of(l, 5 * l, 77, m)
        for want in (48, 49):
            drop = drop_set_with(a, want)
            if drop is None:
                continue
            hit[want] += 1
            records, out, _ = check_calls([b"".join(x for i, x in enumerate(fr) if i not in drop)], what="%d erasures" % want)
            assert records[0]["max_erasures"] == want and records[0]["received"] == a["fcount"] - len(drop)
            assert (out == af and records[0]["flags"] & R.RECOVERED) if want == 48 else (out == b"" and records[0]["flags"] & R.LOST)
    assert hit[48] >= 2 and hit[49] >= 2, hit
    af, fr, a = frags_of(415, 3, 65535, 3)
    assert a["fcount"] * a["plen"] > a["block_bytes"]                              # the last fragments end in padding
    for drop in ((0,), (a["fcount"] - 1,), (0, a["fcount"] - 1)):
        records, out, _ = check_calls([b"".join(x for i, x in enumerate(fr) if i not in drop)])
        assert out == af and records[0]["flags"] == R.FEC | R.ADDR * 0 | R.RECOVERED | R.AF_OK | R.FLUSHED
    hl = a["header_bytes"]
    bad = list(fr)
    bad[5] = flip(bad[5], hl + 3, 4)
    records, out, _ = check_calls([b"".join(bad[1:])])
    assert records[0]["flags"] & R.INCONSISTENT and records[0]["flags"] & R.RECOVERED and not records[0]["flags"] & R.AF_OK and len(out) == 415
    records, out, _ = check_calls([b"".join(bad)])
    assert not records[0]["flags"] & (R.INCONSISTENT | R.RECOVERED | R.AF_OK) and len(out) == 415 and out != af
    # a flipped PARITY byte of a complete group is not judged
    bad = list(fr)
    bad[a["fcount"] - 2] = flip(bad[a["fcount"] - 2], hl + a["plen"] - 1, 0)
    records, out, _ = check_calls([b"".join(bad)])
    assert out == af and records[0]["flags"] == R.FEC | R.AF_OK


def three_packets(m=2, l=140, pseq=65534, **kw):
    return [frags_of(l, 10 + n, (pseq + n) & 0xFFFF, m, **kw) for n in range(3)]


def test_host_reader_order_and_loss(built):
    """Fragments of adjacent Pseq interleaved and reversed; a fragment three packets late; duplicates; a mismatched Fcount;
    Pseq 65534 .. 1 through the wrap; a jump of 1000 against `missing`; 16 late fragments in a row, then recovery; FLUSH."""
    pk = [frags_of(300, n, (65534 + n) & 0xFFFF, 2) for n in range(4)]           # Pseq 65534, 65535, 0, 1
    afs = [p[0] for p in pk]
    inter = [x for pair in zip(pk[0][1], pk[1][1]) for x in pair] + [x for pair in zip(reversed(pk[2][1]), reversed(pk[3][1])) for x in pair]
    records, out, _ = check_calls([b"".join(inter)], what="interleaved")
    assert out == b"".join(afs) and [r["pseq"] for r in records] == [65534, 65535, 0, 1] and all(r["flags"] == R.FEC | R.AF_OK for r in records)
    # a fragment of packet 0 arrives after packets 1, 2, 3: packet 0 was closed by the horizon (recovered), the fragment is late
    late = pk[0][1][1:] + pk[1][1] + pk[2][1] + pk[3][1] + pk[0][1][:1]
    records, out, st = check_calls([b"".join(late)], what="late")
    assert out == b"".join(afs) and records[0]["flags"] & R.RECOVERED and st["totals"]["late"] == 1
    # duplicates and a fragment that claims another Fcount
    f0 = pk[0][1]
    liar = R.header(65534, 1, len(f0) + 1, 20, (pk[0][2]["rs_k"], pk[0][2]["rs_z"])) + bytes(20)
    records, out, st = check_calls([b"".join([f0[0], f0[0], liar, f0[1], f0[1]] + f0[2:])], what="duplicates")
    assert out == afs[0] and st["totals"]["duplicates"] == 2 and st["totals"]["mismatched"] == 1 and records[0]["flags"] == R.FEC | R.AF_OK
    # a jump of 1000: the group in between is closed (LOST: one fragment of it), 998 more are missing
    far = frags_of(300, 9, (65534 + 1000) & 0xFFFF, 2)
    records, out, st = check_calls([b"".join(pk[0][1] + pk[1][1][:1] + far[1])], what="jump")
    assert [r["pseq"] for r in records] == [65534, 65535, 998] and records[1]["flags"] & R.LOST and st["totals"]["missing"] == 998
    assert out == afs[0] + far[0]
    # 16 late fragments are dropped, the 17th starts afresh: the open group is closed first
    old = frags_of(300, 5, 60000, 8)
    assert old[2]["fcount"] >= 34
    stream = pk[2][1] + pk[3][1][:3] + old[1][:17] + old[1][17:]
    records, out, st = check_calls([b"".join(stream)], what="late run")
    assert st["totals"]["late"] == 16 and [r["pseq"] for r in records] == [0, 1, 60000] and records[1]["flags"] & R.LOST
    assert records[2]["received"] == old[2]["fcount"] - 16 and records[2]["flags"] & R.FLUSHED
    # FLUSH closes both open groups in order, and an empty call with FLUSH does it too
    records, out, st = check_calls([b"".join(pk[0][1][2:] + pk[1][1][1:]), b""], what="flush")
    assert [r["flags"] & (R.FLUSHED | R.RECOVERED) for r in records] == [R.FLUSHED | R.RECOVERED] * 2 and out == afs[0] + afs[1]
    records, out, st = check_calls([b"".join(pk[1][1][1:])], flush_last=False)
    assert records == [] and st["groups"][65535]["frags"]
    records, out, st = check_calls([b"".join(pk[1][1][1:]), b""], what="flush of the far group alone")
    assert out == afs[1] and st["totals"]["missing"] == 0 and st["horizon"] == 65535


def damaged_stream():
    """three packets with everything a byte stream can suffer, and one packet without FEC and one with Addr between"""
    pk = three_packets()
    plain = frags_of(700, 50, 1, fec=False, max_payload=100)
    addr = frags_of(208, 51, 2, 3, addr=True)
    f = [list(p[1]) for p in pk] + [list(plain[1]), list(addr[1])]
    f[0][1] = b"\x00garbage" + f[0][1]                                            # garbage between fragments
    f[0][3] = f[0][3][:9] + f[0][3][10:]                                          # a byte gone
    f[1][0] = flip(f[1][0], 5, 0)                                                 # a plausible header with a wrong HCRC
    f[1][2] = f[1][2][:20] + b"PF" + f[1][2][22:]                                 # "PF" inside a payload
    f[2][1] = b"PF" + f[2][1]                                                     # "PF" in front of a header
    f[3][2], f[3][4] = f[3][4], f[3][2]
    del f[3][5]                                                                   # without FEC: LOST
    return b"".join(b"".join(x) for x in f) + b"PF\x00"


def test_host_reader_streams(built):
    """Garbage between fragments, a byte gone, a wrong HCRC, "PF" inside a payload, FEC and non-FEC and Addr in one call; a
    complete fragment nested in a payload stays payload."""
    data = damaged_stream()
    records, out, st = check_calls([data], what="damaged")
    t = st["totals"]
    assert t["skipped"] > 0 and t["resyncs"] >= 3 and t["lost"] == 1 and t["recovered"] >= 2 and len(st["tail"]) == 3
    assert [bool(r["flags"] & R.FEC) for r in records] == [True, True, True, False, True] and records[4]["flags"] & R.ADDR
    assert records[4]["source"] == 0x1234 and records[4]["dest"] == 0xABCD
    inner = frags_of(12, 1, 7, 1)[1][0]
    af = make_af(400, 3, 9)
    af = af[:100] + inner + af[100 + len(inner):-2]
    af += R.crc16(af).to_bytes(2, "big")
    a = R.layout(400, False, 0, 400, False)
    records, out, st = check_calls([b"".join(R.fragments(af, a, 9))], what="nested")
    assert out == af and st["totals"]["fragments"] == 1 and records[0]["flags"] == R.AF_OK
    # without FEC: fragments in any order, the last first
    a = R.layout(700, False, 0, 100, False)
    fr = R.fragments(make_af(700, 8, 3), a, 3)
    records, out, st = check_calls([b"".join(fr[::-1])], what="reversed without FEC")
    assert out == make_af(700, 8, 3) and records[0]["flags"] == R.AF_OK | R.FLUSHED * 0 and records[0]["plen"] == 100


def test_cut_at_every_byte_of_three_packets(built):
    data = b"".join(b"".join(p[1]) for p in three_packets(m=1, l=60))
    want = check_calls([data], what="whole")
    assert len(want[0]) == 3 and want[1] == b"".join(p[0] for p in three_packets(m=1, l=60))
    for cut in range(len(data) + 1):
        got = check_calls([data[:cut], data[cut:]], what="cut at %d" % cut)
        assert got[0] == want[0] and got[1] == want[1] and got[2]["totals"] == want[2]["totals"], cut


def test_random_cuts_and_many_pieces_of_a_damaged_stream(built):
    data = damaged_stream()
    want = check_calls([data], what="whole")
    rng = np.random.default_rng(4)
    for trial in range(50):
        cuts = sorted(rng.integers(0, len(data) + 1, int(rng.integers(1, 30))).tolist())
        cuts += cuts[:2]                                                          # ... calls of no bytes
        edges = [0] + sorted(cuts) + [len(data)]
        got = check_calls([data[a:b] for a, b in zip(edges, edges[1:])], what="trial %d" % trial)
        assert got[0] == want[0] and got[1] == want[1] and got[2]["totals"] == want[2]["totals"], trial


def hostile_states():
    rng = np.random.default_rng(9)
    _, _, st = check_calls([b"".join(three_packets()[0][1][1:4])], flush_last=False)
    good = R.pack_state(st)
    states = [np.full(STATE_BYTES, 0xFF, np.uint8), rng.integers(0, 256, STATE_BYTES, dtype=np.uint8)]
    for field, value in (("kind", 3), ("fcount", 0), ("fcount", 300), ("s", 9000), ("received", 2), ("chunks", 41), ("length", 11), ("rs_k", 208),
                         ("last_len", 5), ("pseq", 7), ("have_s", 0), ("map", 1 << 40)):
        s = good.copy()
        g = s[R.HEAD_BYTES + (65534 & 1) * R.GROUP_BYTES:][:64].view(R.GROUP_DTYPE)
        g[field] = value
        states.append(s)
    s = good.copy()
    s[:R.HEAD_BYTES].view(R.HEAD_DTYPE)["tail_bytes"] = 1 << 31
    s[:R.HEAD_BYTES].view(R.HEAD_DTYPE)["late_run"] = 200
    states.append(s)
    return good, states, st


def test_hostile_state_record_reads_nothing_outside(built):
    """Records this code did not write: the call ends, counts stay inside their bounds, and a group head that is not
    consistent is an empty group (the carried fragments are gone, the rest of the stream is read as ever)."""
    good, states, st = hostile_states()
    rest = b"".join(three_packets()[0][1][4:])
    emptied = R.read(dict(st, groups={}), rest, True)                              # the same head, no carried group
    assert emptied[2]["lost"] == 1 and emptied[2]["packets"] == 0
    base = run_host([Case(rest, good, True)])[0]
    assert base["result"]["packets"] == 1 and base["records"][0]["flags"] & R.AF_OK
    for i, s in enumerate(states):
        got = run_host([Case(rest, s, True)])[0]
        res = got["result"]
        assert res["records"] <= dabgpu.pft_read_max_records(len(rest)) and res["out_bytes"] <= dabgpu.pft_read_out_bytes(len(rest)), i
        assert res["tail_bytes"] <= 8211 and (got["out"][int(res["out_bytes"]):] == FILL).all(), i
        if 2 <= i < len(states) - 1:                                              # one field of the carried group's head is wrong
            assert_is_reference(got, emptied, "hostile state %d" % i)


def test_refused_calls_write_nothing(built):
    data = b"".join(three_packets()[0][1])

    def refused(change):
        c = Case(data)
        entries = host_entries([c])
        change(entries[0], c)
        with pytest.raises(dabgpu.DabGpuError):
            dabgpu.pft_read_host(entries)
        return all((c.arrays[k] == FILL).all() for k in ("state_out", "out", "records", "result"))
    assert refused(lambda e, c: setattr(e, "n_bytes", -1)) and refused(lambda e, c: setattr(e, "n_bytes", (1 << 30) + 1))
    assert refused(lambda e, c: setattr(e, "d_bytes", None)) and refused(lambda e, c: setattr(e, "flags", 2))
    for field in ("d_state_out", "d_out", "d_records", "d_result"):
        assert refused(lambda e, c: setattr(e, field, None)), field
    for field, off in (("d_bytes", 8), ("d_state_out", 8), ("d_out", 4), ("d_records", 2), ("d_result", 1)):
        assert refused(lambda e, c: setattr(e, field, getattr(e, field) + off)), field
    assert refused(lambda e, c: setattr(e, "d_state_in", e.d_state_out + 16))
    good, bad = Case(data), Case(data)
    entries = host_entries([good, bad])
    entries[1].d_result = None
    with pytest.raises(dabgpu.DabGpuError):
        dabgpu.pft_read_host(entries)
    assert (good.arrays["result"] == FILL).all() and (good.arrays["state_out"] == FILL).all()
    assert dabgpu.lib().dabgpu_pft_read_host(None, 1) == -1 and dabgpu.lib().dabgpu_pft_read_host(None, 0) == 0


def test_unsupported_groups(built):
    """Fcount * s > MAX_BLOCK, c < 1, c > 40, l < 12, l > 8192: every fragment counts in `unsupported`, the group gives no
    record and is `missing` when the horizon passes it."""
    ok = frags_of(140, 1, 13, 2)
    for n, (fcount, plen, fec) in enumerate(UNSUPPORTED):
        frs = [R.header(10, g, fcount, plen, fec) + bytes(plen) for g in (0, 1 if fcount > 1 else 0)]
        records, out, st = check_calls([b"".join(frs + ok[1])], what="unsupported %d" % n)
        assert st["totals"]["unsupported"] == 2 and st["totals"]["missing"] == 3 and [r["pseq"] for r in records] == [13] and out == ok[0], n


def test_round_trip_to_the_edi_reader(built):
    """edi_reference packets -> PFT writer -> fragments dropped -> PFT reader -> dabgpu_edi_read_host: the rows of the
    undamaged stream, with `gap` counted where a packet is LOST."""
    import test_edi_read as E
    from test_eti import CONFIGS
    pk, _ = E.make_packets("one_eep_a", 12, 4, start=100, seq=65530)
    a = R.layout(len(pk[0]), True, 2, 1400, False)
    frs = dabgpu.pft_fragments_host(lib_layout(a), np.frombuffer(b"".join(pk), np.uint8)[None], [65530])[0].tobytes()
    fb, f = a["header_bytes"] + a["plen"], a["fcount"]
    frags = [[frs[(n * f + g) * fb:(n * f + g + 1) * fb] for g in range(f)] for n in range(12)]
    rng = np.random.default_rng(2)
    for n in range(12):
        lose = a["guaranteed_losses"] if n != 7 else f - 2                        # packet 7 cannot come back
        for g in sorted(rng.choice(f, lose, replace=False).tolist(), reverse=True):
            del frags[n][g]
    got = run_host([Case(b"".join(b"".join(x) for x in frags), None, True)])[0]
    n_out = int(got["result"]["out_bytes"])
    assert got["result"]["packets"] == 11 and got["result"]["lost"] == 1 and got["result"]["recovered"] == 11
    assert got["out"][:n_out].tobytes() == b"".join(p for n, p in enumerate(pk) if n != 7)
    streams = CONFIGS["one_eep_a"]()
    rows = E.run_host([E.Case(streams, got["out"][:n_out].tobytes())])[0]
    whole = E.run_host([E.Case(streams, b"".join(pk))])[0]
    assert rows["result"]["rows"] == 11 and rows["result"]["gap_sum"] == 1 and whole["result"]["rows"] == 12
    keep = [n for n in range(12) if n != 7]
    assert rows["fib"][:11].tobytes() == whole["fib"][keep].tobytes() and rows["outs"][0][:11].tobytes() == whole["outs"][0][keep].tobytes()
    assert list(rows["status"]["gap"][:11]) == [0] * 7 + [1] + [0] * 3 and list(rows["status"]["dlfc"][:11]) == list(whole["status"]["dlfc"][keep])


def test_fuzz_program_under_sanitizers(built, tmp_path):
    """tests/pft_fuzz.cpp: the header alone, under AddressSanitizer and UBSan, on damaged streams whole and in pieces and on
    hostile state records."""
    exe = tmp_path / "pft_fuzz"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pft_fuzz.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), "300"], text=True)
    assert "pft_fuzz ok" in out, out


def test_mirror_reads_a_pft_stream_in_uneven_pieces(built, tmp_path):
    """tests/pft_mirror_check.cpp, under AddressSanitizer and UBSan: BasicRadio::ProcessPft over the TEST-ONLY fake ABI
    (unchanged: no new symbol).  The EDI mirror test's ensemble as PF fragments, guaranteed_losses of every packet's missing and
    the rest of every packet reversed, fed in uneven pieces: what ProcessEdi shows on the AF packets themselves."""
    from test_edi_read import HOST, mirror_stream
    fake, oracle = os.path.join(ROOT, "tests", "fake_abi"), os.path.join(ROOT, "oracle")
    assert "pft" not in open(os.path.join(fake, "fake_dabgpu.cpp")).read()
    exe = str(tmp_path / "pft_mirror_check")
    srcs = [os.path.join(ROOT, "tests", "pft_mirror_check.cpp"), os.path.join(fake, "fake_dabgpu.cpp")]
    srcs += [os.path.join(HOST, s) for s in ("ofdm/ofdm_demodulator.cpp", "basic_radio/basic_radio.cpp", "basic_radio/basic_dab_plus_channel.cpp", "dab/fic/fic_parser.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I" + HOST,
                           "-I" + os.path.join(ROOT, "include"), "-I" + oracle, "-I" + fake] + srcs +
                          ["-L" + oracle, "-loracle", "-Wl,-rpath," + oracle, "-o", exe])
    _, pk, _, _ = mirror_stream()
    a = R.layout(len(pk[0]), True, 2, 1400, False)
    rng = np.random.default_rng(6)
    stream = b""
    for n, p in enumerate(pk):
        fr = R.fragments(p, a, 65500 + n)
        for g in sorted(rng.choice(a["fcount"], a["guaranteed_losses"], replace=False).tolist(), reverse=True):
            del fr[g]
        stream += b"".join(fr[::-1])

    def run(mode, data, pieces):
        path = tmp_path / ("in." + mode)
        path.write_bytes(data)
        r = subprocess.run([exe, mode, str(path)] + [str(x) for x in pieces], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.splitlines()
    want = run("edi", b"".join(pk), [len(pk[0])])
    got = run("pft", stream, [1000, 1, 77, 5000])
    assert got[1:] == want[1:] and "rows=%d " % len(pk) in got[1] and "skipped=0 " in got[1], (got[:3], want[:3])
    assert got[0].startswith("pft records=%d packets=%d lost=0 recovered=%d " % (len(pk), len(pk), len(pk))), got[0]


def test_edi_play_reads_a_pft_file_on_the_host(built, tmp_path):
    """tools/edi_play.py --host --pft (no GPU: pft_read_host in front of edi_read_host) on the mirror test's packets as fragments,
    guaranteed_losses of every packet's missing: what it lists from the AF packets themselves, and the PFT reader's counters."""
    import sys
    from test_edi_read import mirror_stream
    _, pk, _, _ = mirror_stream()
    a = R.layout(len(pk[0]), True, 1, 500, False)
    rng = np.random.default_rng(8)
    stream = b""
    for n, p in enumerate(pk):
        fr = R.fragments(p, a, n)
        for g in sorted(rng.choice(a["fcount"], a["guaranteed_losses"], replace=False).tolist(), reverse=True):
            del fr[g]
        stream += b"".join(fr)
    outs = []
    for name, data, extra in (("in.edi", b"".join(pk), []), ("in.pft", stream, ["--pft"])):
        (tmp_path / name).write_bytes(data)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "edi_play.py"), "--host", "--chunk-bytes", "7001", str(tmp_path / name)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(r.stdout.splitlines())
    assert outs[1][1:] == outs[0] and "rows=%d " % len(pk) in outs[0][-1]
    pft = dict(kv.split("=") for kv in outs[1][0].split()[1:])
    assert (pft["packets"], pft["recovered"], pft["lost"], pft["skipped"], pft["tail_bytes"]) == (str(len(pk)), str(len(pk)), "0", "0", "0"), pft


def test_kernels_use_no_scratch_and_spill_nothing(built, tmp_path):
    """The method of test_edi_read.py on the two new code objects: no scratch, no spills, no accumulation registers.  The walk
    kernel holds the two open groups (2 x 10496 bytes) in LDS per single-wave workgroup: 160 KB / 21.3 KB lets 7 of them share
    a CU, two waves per SIMD, which at most 128 VGPRs a lane admit twice over."""
    from test_device_asm import kernel_metadata
    csrc, tools = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "csrc"), "/opt/rocm/lib/llvm/bin/"
    found = {}
    for name in ("pft_kernels", "pft_read_kernels"):
        obj = os.path.join(csrc, name + ".o")
        if not os.path.exists(obj):
            subprocess.check_call(["make", "-C", csrc, name + ".o"], stdout=subprocess.DEVNULL)
        fat, co = str(tmp_path / (name + ".fat")), str(tmp_path / (name + ".co"))
        subprocess.check_call([tools + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([tools + "clang-offload-bundler", "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + fat, "--output=" + co])
        found.update(kernel_metadata(subprocess.check_output([tools + "llvm-readelf", "--notes", co], text=True)))
    assert sorted(k.split("pft_")[1].split("_kernel")[0] for k in found) == ["fragments", "read_check", "read_fill", "read_walk"], list(found)
    for k, v in found.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v.get("agpr_count", 0) == 0 and v["vgpr_count"] <= 128, (k, v)
    by = lambda part: [v for k, v in found.items() if part in k][0]
    assert by("read_walk")["group_segment_fixed_size"] <= 160 * 1024 // 7
    assert by("read_check")["vgpr_count"] <= 64 and by("read_check")["group_segment_fixed_size"] == 0          # 8 waves per SIMD
    assert by("read_fill")["vgpr_count"] <= 64 and by("read_fill")["group_segment_fixed_size"] <= 160 * 1024 // 8
    assert by("fragments")["vgpr_count"] <= 64 and by("fragments")["group_segment_fixed_size"] <= 160 * 1024 // 8


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def rctx(built):
    from conftest import make_ctx
    c = make_ctx(None, max_frames=64)
    yield c
    c.close()


def run_dev(ctx, cases):
    import torch
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    full = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    for c in cases:
        c.arrays = {"bytes": dev(np.frombuffer(c.data or b"\0", np.uint8).copy()), "state_in": None if c.state is None else dev(c.state),
                    "state_out": full(STATE_BYTES), "out": full(c.n_out), "records": full(c.n_rec * 32), "result": full(64)}
    ctx.pft_read_dev([_entry(c, lambda x: x.data_ptr()) for c in cases])
    ctx.sync()
    return [_collect(c, lambda x: x.cpu().numpy()) for c in cases]


def assert_same(a, b, what=""):
    for k in ("result", "records", "out", "state"):
        x, y = np.atleast_1d(a[k]).view(np.uint8).reshape(-1), np.atleast_1d(b[k]).view(np.uint8).reshape(-1)
        if x.tobytes() != y.tobytes():
            bad = np.nonzero(x != y)[0]
            pytest.fail("%s %s differs at bytes %s (%d in all): %s / %s" % (what, k, bad[:8], bad.size, a["result"], b["result"]))


def assert_device_is_host(ctx, make_cases, what=""):
    want, got = run_host(make_cases()), run_dev(ctx, make_cases())
    for i, (w, g) in enumerate(zip(want, got)):
        assert_same(g, w, "%s entry %d" % (what, i))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("n_streams,n_packets", [(1, 1), (3, 5)])
def test_device_writer_is_the_host_writer(rctx, n_streams, n_packets):
    """l in {12, 207, 208, 415, 8192} x m in {0, 2} x FEC / no FEC, 1 and 3 streams, 1 and 5 packets from Pseq 65533 on, so
    that pseq_start wraps; the bytes between the streams stay as they were."""
    import torch
    for l in (12, 207, 208, 415, 8192):
        for m, fec in ((0, True), (2, True), (0, False)):
            a = R.layout(l, fec, m, 1400 if fec else 97, fec and l == 415)
            lay = lib_layout(a)
            af = np.stack([np.frombuffer(b"".join(make_af(l, 31 * s + n, n) for n in range(n_packets)), np.uint8) for s in range(n_streams)])
            pseq = [65533 + 7 * s for s in range(n_streams)]
            want = dabgpu.pft_fragments_host(lay, af, pseq, 0x1234, 0xABCD)
            in_stride, out_stride = (af.shape[1] + 15) // 16 * 16 + 16, (want.shape[1] + 15) // 16 * 16 + 32
            src = np.zeros((n_streams, in_stride), np.uint8)
            src[:, :af.shape[1]] = af
            d_src, d_dst = torch.from_numpy(src).cuda(), torch.full((n_streams, out_stride), FILL, dtype=torch.uint8, device="cuda")
            rctx.pft_fragments_dev(lay, n_streams, n_packets, d_src.data_ptr(), in_stride, d_dst.data_ptr(), out_stride, pseq, 0x1234, 0xABCD)
            rctx.sync()
            got = d_dst.cpu().numpy()
            assert got[:, :want.shape[1]].tobytes() == want.tobytes(), (l, m, fec)
            assert (got[:, want.shape[1]:] == FILL).all(), (l, m, fec)
    if n_streams == 1:
        got = rctx.pft_fragments(lib_layout(R.layout(140, True, 2)), torch.from_numpy(np.frombuffer(make_af(140, 1), np.uint8).copy()[None]).cuda(), [5])
        assert got.cpu().numpy().tobytes() == b"".join(R.fragments(make_af(140, 1), R.layout(140, True, 2), 5))


def erasure_count_streams():
    """c = 2, k = 12, one block byte per fragment (f = 120, s = 1): 1, 2, 47, 48 and 49 erasures in chunk 0, none in chunk 1"""
    af = make_af(24, 8, 3)
    chunk0 = list(range(12)) + list(range(24, 72))                                # the block indexes of chunk 0
    return [b"".join(custom_frags(af, 2, 12, 120, 1, 3, chunk0[5:5 + e])) for e in (1, 2, 47, 48, 49)], af


def graded_stream():
    """c = 40 with a different erasure count in every chunk: k = 6, f = 241, s = 9 and a fixed set of lost fragments (the
    interleave spreads a lost fragment over all chunks alike; this layout and set were searched for)"""
    af = make_af(40 * 6 - 3, 12, 9)
    return b"".join(custom_frags(af, 40, 6, 241, 9, 9, GRADED_DROP)), af, GRADED_DROP


GRADED_DROP = [0, 1, 2, 3, 5, 6, 7, 8, 10, 12, 13, 14, 15, 16, 17, 18, 19, 21, 22, 24, 26, 27, 28, 29, 31, 33, 34, 35, 36, 38,
               41, 44, 46, 53, 56, 60, 62, 65, 67, 74, 76, 82, 83, 84, 88, 89, 91, 94, 96, 97, 99, 101, 102, 103, 104, 105,
               106, 107, 108, 109, 110, 111, 114, 115, 116, 117, 118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129,
               130, 131, 132, 133, 134, 136, 137, 138, 139, 140, 141, 143, 145, 149, 153, 158, 159, 164, 166, 168, 169, 170,
               171, 172, 174, 175, 176, 179, 180, 181, 182, 185, 194, 195, 197, 198, 224, 232, 233]


UNSUPPORTED = ((42, 250, (207, 0)), (2, 20, (1, 0)), (200, 50, (1, 0)), (1, 60, (12, 1)), (41, 255, (207, 0)), (106, 100, None))


def device_cases(loss_cases):
    """Every loss / order / stream case of the CPU tests as (stream, FLUSH) entries of one call.  Thinned for time, and only
    there: of the 560 three-fragment sets of the 8192-byte packet every ninth (the ones the CPU test holds to the Python
    reference too); its whole fragment set, every single loss and every other size's every set are all here."""
    pk = [frags_of(300, n, (65534 + n) & 0xFFFF, 2) for n in range(4)]
    afs = [p[0] for p in pk]
    old = frags_of(300, 5, 60000, 8)
    far = frags_of(300, 9, (65534 + 1000) & 0xFFFF, 2)
    inter = [x for pair in zip(pk[0][1], pk[1][1]) for x in pair] + [x for pair in zip(reversed(pk[2][1]), reversed(pk[3][1])) for x in pair]
    f0 = pk[0][1]
    liar = R.header(65534, 1, len(f0) + 1, 20, (pk[0][2]["rs_k"], pk[0][2]["rs_z"])) + bytes(20)
    inner = frags_of(12, 1, 7, 1)[1][0]
    nested = make_af(400, 3, 9)
    nested = nested[:100] + inner + nested[100 + len(inner):-2]
    nested += R.crc16(nested).to_bytes(2, "big")
    order = [b"".join(inter),                                                                   # interleaved and reversed
             b"".join(pk[0][1][1:] + pk[1][1] + pk[2][1] + pk[3][1] + pk[0][1][:1]),            # three packets late
             b"".join([f0[0], f0[0], liar, f0[1], f0[1]] + f0[2:]),                             # duplicates, a mismatched Fcount
             b"".join(pk[0][1] + pk[1][1][:1] + far[1]),                                        # a jump of 1000
             b"".join(pk[2][1] + pk[3][1][:3] + old[1]),                                        # 16 late fragments in a row
             b"".join(pk[0][1][2:] + pk[1][1][1:]),                                             # FLUSH closes two groups
             b"".join(pk[1][1][1:]),                                                            # ... the far group alone
             damaged_stream(), b"",
             b"".join(R.fragments(nested, R.layout(400, False, 0, 400, False), 9)),             # a complete fragment nested in a payload
             b"".join(R.fragments(make_af(700, 8, 3), R.layout(700, False, 0, 100, False), 3)[::-1])]   # without FEC, the last index first
    entries = [(data, True) for data, _, through_reference in loss_cases.values() if through_reference]
    entries += [(s, True) for s in order] + [(s, False) for s in order]
    entries += [(s, True) for s in erasure_count_streams()[0] + [graded_stream()[0]]]
    for l, m in ((8192, 2), (415, 8), (2476, 5)):
        af, fr, a = frags_of(l, 5 * l, 77, m)
        drops = [d for d in (drop_set_with(a, want) for want in (48, 49)) if d is not None]
        entries += [(b"".join(x for i, x in enumerate(fr) if i not in drop), True) for drop in drops]
    af, fr, a = frags_of(415, 3, 65535, 3)
    bad = list(fr)
    bad[5] = flip(bad[5], a["header_bytes"] + 3, 4)
    entries += [(s, True) for s in (b"".join(bad[1:]), b"".join(bad), b"".join(fr[1:]), b"".join(fr[:-1]), b"".join(fr[1:-1]))]
    for fcount, plen, fec in UNSUPPORTED:
        frs = [R.header(10, g, fcount, plen, fec) + bytes(plen) for g in (0, 1 if fcount > 1 else 0)]
        entries.append((b"".join(frs + frags_of(140, 1, 13, 2)[1]), True))
    return entries


@pytest.mark.gpu
def test_device_all_cases_in_one_call(rctx, loss_cases):
    entries = device_cases(loss_cases)
    want = assert_device_is_host(rctx, lambda: [Case(s, None, flush) for s, flush in entries])
    total = lambda k: sum(int(w["result"][k]) for w in want)
    assert total("recovered") > 300 and total("lost") >= 6 and total("duplicates") >= 4 and total("mismatched") >= 2 and total("late") >= 17
    assert total("unsupported") == 12 and total("missing") >= 998 and len(entries) > 400
    assert sum("l=8192" in name and through for name, (_, _, through) in loss_cases.items()) >= 2 + 24 + 63


@pytest.mark.gpu
def test_device_erasure_counts_in_one_chunk(rctx):
    """1, 2, 47, 48 and 49 erasures in one chunk while its neighbour has none; c = 40 with a different count in every chunk"""
    streams, af = erasure_count_streams()
    want = assert_device_is_host(rctx, lambda: [Case(s, None, True) for s in streams])
    for w, e in zip(want, (1, 2, 47, 48, 49)):
        r = w["records"][0]
        assert r["max_erasures"] == e and r["chunks"] == 2 and (w["result"]["chunks_filled"], w["result"]["bytes_filled"]) == ((1, e) if e < 49 else (0, 0))
        assert (w["out"][:24].tobytes() == af and r["flags"] & R.AF_OK) if e < 49 else r["flags"] & R.LOST
    stream, af, drop = graded_stream()
    counts = R.chunk_counts(40, 6, 241)[:, drop].sum(1)
    assert counts.max() <= 48 and len(set(counts.tolist())) == 40
    w = assert_device_is_host(rctx, lambda: [Case(stream, None, True)])[0]
    assert w["out"][:len(af)].tobytes() == af and w["result"]["bytes_filled"] == counts.sum() and w["records"][0]["max_erasures"] == counts.max()


@pytest.mark.gpu
@pytest.mark.parametrize("n_entries", [1, 64, 65])
def test_device_entry_counts(rctx, n_entries):
    """1, 64 and 65 entries, every fifth of 0 bytes, every entry its own packets and losses"""
    def make():
        cases = []
        for i in range(n_entries):
            af, fr, a = frags_of(100 + 37 * i, i, 1000 * i, i % 4)
            keep = [x for g, x in enumerate(fr) if g != i % a["fcount"] or i % 2]
            cases.append(Case(b"" if i % 5 == 4 else b"".join(keep), None, True))
        return cases
    want = assert_device_is_host(rctx, make)
    assert sum(int(w["result"]["packets"]) for w in want) == n_entries - n_entries // 5


@pytest.mark.gpu
def test_device_130_packets_of_one_entry(rctx):
    pk = [frags_of(200 + n % 7, n, (65500 + n) & 0xFFFF, 2) for n in range(130)]
    data = b"".join(b"".join(x for g, x in enumerate(p[1]) if (g + n) % 9) for n, p in enumerate(pk))
    w = assert_device_is_host(rctx, lambda: [Case(data, None, True)])[0]
    assert w["result"]["packets"] == 130 and w["out"][:int(w["result"]["out_bytes"])].tobytes() == b"".join(p[0] for p in pk)


@pytest.mark.gpu
def test_device_lengths_around_the_check_span(rctx):
    """|S| on both sides of the 4096 positions a workgroup of the check launch judges, and of its 64-position words"""
    pk = [frags_of(500, n, n, 1) for n in range(12)]
    data = b"".join(b"".join(p[1]) for p in pk)
    assert len(data) > 8300
    assert_device_is_host(rctx, lambda: [Case(data[:n], None, n % 2 == 0) for n in (63, 64, 65, 4095, 4096, 4097, 4110, 8191, 8192, 8193, len(data))])


@pytest.mark.gpu
def test_device_rejects_a_flip_in_each_header_byte(rctx):
    """every bit of every byte of one header (20 bytes: FEC and Addr), each in an entry of its own: the HCRC rejects them all"""
    af, fr, a = frags_of(140, 2, 500, 2, addr=True)
    assert a["header_bytes"] == 20
    streams = [b"".join(fr[:2] + [flip(fr[2], pos, bit)] + fr[3:]) for pos in range(20) for bit in range(8)]
    want = assert_device_is_host(rctx, lambda: [Case(s, None, True) for s in streams])
    for w in want:
        assert w["result"]["fragments"] == a["fcount"] - 1 and w["result"]["skipped"] == len(fr[2]) and w["result"]["recovered"] == 1


@pytest.mark.gpu
def test_device_two_calls_with_the_carry_equal_the_host_calls(rctx, loss_cases):
    """a damaged stream, open groups closed by an empty call with FLUSH, and hostile state records: the first call's state
    goes into the second on each side"""
    data = damaged_stream()
    good, states, _ = hostile_states()
    cuts = [0, 1, 17, 300, len(data) // 2, len(data) - 1, len(data)]
    first = assert_device_is_host(rctx, lambda: [Case(data[:c], None, False) for c in cuts], "first call")
    assert_device_is_host(rctx, lambda: [Case(data[c:], f["state"], True) for c, f in zip(cuts, first)], "second call")
    pk = [frags_of(300, n, (65534 + n) & 0xFFFF, 2) for n in range(2)]
    opened = [b"".join(pk[0][1][2:] + pk[1][1][1:]), b"".join(pk[1][1][1:])]          # two open groups; the far one alone
    first = assert_device_is_host(rctx, lambda: [Case(s, None, False) for s in opened], "groups left open")
    assert all(int(f["result"]["records"]) == 0 for f in first)
    second = assert_device_is_host(rctx, lambda: [Case(b"", f["state"], True) for f in first], "an empty call with FLUSH")
    assert [int(w["result"]["recovered"]) for w in second] == [2, 1] and second[1]["out"][:300].tobytes() == pk[1][0]
    rest = b"".join(three_packets()[0][1][4:])
    assert_device_is_host(rctx, lambda: [Case(rest, s, True) for s in [good] + states], "hostile states")


@pytest.mark.gpu
def test_device_refused_calls_write_nothing(rctx):
    import torch
    data = b"".join(three_packets()[0][1])
    cases = [Case(data), Case(data)]
    full = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    for c in cases:
        c.arrays = {"bytes": torch.from_numpy(np.frombuffer(c.data, np.uint8).copy()).cuda(), "state_in": None, "state_out": full(STATE_BYTES),
                    "out": full(c.n_out), "records": full(c.n_rec * 32), "result": full(64)}
    entries = [_entry(c, lambda x: x.data_ptr()) for c in cases]
    entries[1].d_out += 8
    with pytest.raises(dabgpu.DabGpuError):
        rctx.pft_read_dev(entries)
    rctx.sync()
    for c in cases:
        assert all((c.arrays[k].cpu().numpy() == FILL).all() for k in ("state_out", "out", "records", "result"))


@pytest.mark.gpu
def test_device_round_trip_to_the_edi_rows_and_the_follow_call(rctx):
    """Decode buffers -> dabgpu_edi_frames_dev -> dabgpu_pft_fragments_dev -> fragments lost -> dabgpu_pft_read_dev ->
    dabgpu_edi_read_dev: the sub-channel rows that went in; and dabgpu_dabplus_follow_dev finds on them the access units it
    finds on the buffers that went into the writer (the closing step of tests/test_edi_read.py)."""
    import torch
    from dabgpu import synth
    from test_edi import run_edi
    from test_eti import SERVICES
    from test_eti_read import make_fibs
    ens = synth.ServiceEnsemble(7, SERVICES[:1], n_frames=10, extras=False)
    streams = [(3, dabgpu.subchannel(0, 64, level=3))]
    n_cif = 40
    lf = np.ascontiguousarray(np.asarray(ens.msc_bytes[0], np.uint8)[:n_cif]).reshape(1, n_cif, 192)
    fib, ok = make_fibs(np.random.default_rng(1), n_cif)
    edi, _, _, packet = run_edi(rctx, streams, fib[None], ok[None], [lf], cif_start=[4990], seq_start=[65530], slack=0)
    lay = dabgpu.pft_layout(packet, True, 2)
    stride = (n_cif * packet + 15) // 16 * 16
    src = np.zeros((1, stride), np.uint8)
    src[0, :n_cif * packet] = edi[0, :n_cif * packet]
    pf_bytes = rctx.pft_fragments(lay, torch.from_numpy(src).cuda()[:, :n_cif * packet], [65530]).cpu().numpy()[0]
    fb = lay.header_bytes + lay.plen
    rng = np.random.default_rng(3)
    kept = b"".join(pf_bytes[(n * lay.fcount + g) * fb:(n * lay.fcount + g + 1) * fb].tobytes() for n in range(n_cif)
                    for g in np.sort(rng.choice(lay.fcount, lay.fcount - lay.guaranteed_losses, replace=False)))
    data = np.zeros((len(kept) + 15) // 16 * 16, np.uint8)
    data[:len(kept)] = np.frombuffer(kept, np.uint8)
    out, records, result, _ = rctx.pft_read(torch.from_numpy(data[:len(kept)].copy()).cuda()[None], flush=True)
    res = result.cpu().numpy().view(RES).reshape(-1)[0]
    n_out = int(res["out_bytes"])                                                 # (the one word that has to reach the host)
    assert res["packets"] == n_cif == res["recovered"] and n_out == n_cif * packet
    assert out.cpu().numpy()[0, :n_out].tobytes() == edi[0, :n_cif * packet].tobytes()
    af = torch.zeros((1, (n_out + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
    af[0, :n_out] = out[0, :n_out]
    _, _, outs, _, eres, _ = rctx.edi_read(af[:, :n_out].contiguous() if n_out % 16 == 0 else af, streams)
    eres = eres.cpu().numpy().view(dabgpu.EDI_READ_RESULT_DTYPE).reshape(-1)[0]
    assert int(eres["rows"]) == n_cif and not eres["gap_sum"] and outs[0].cpu().numpy()[0, :n_cif].tobytes() == lf.tobytes()

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
