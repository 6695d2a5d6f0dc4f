"""dabgpu_pad_labels_dev / dabgpu_pad_labels_host (the dynamic label of every followed DAB+ service, from the PAD of its
access units) and dabgpu_pad_label_utf8, against tests/pad_reference.py: labels, counters byte for byte and count for
count -- no tolerance anywhere -- every output between sentinel bytes.

The cases are eight streams of at most 12 super-frames (STREAMS), each a sequence of scenarios that begin on a super-frame:
the CPU tests feed them scenario by scenario through dabgpu_pad_labels_host and check what each scenario is about; the GPU
test takes all eight in one ragged call.  The transmit side is dabgpu/synth.py's, written from the same clauses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
from dabgpu import synth

import pad_reference as P
from conftest import ROOT
from test_device_asm import CSRC, kernel_metadata

ARG, PROFILE, CAPACITY = -1, -5, -6
FILL, GAP = 0xA7, 64
KINDS = {2: (0, 1), 3: (1, 1), 4: (0, 0), 6: (1, 0)}                 # access units per super-frame -> (dac_rate, sbr)
FIRST = {2: 5, 3: 6, 4: 8, 6: 11}
NO_PAD = b"\x21"                                                      # a channel pair element in front: no PAD
RANDOM = "random"                                                     # the body build_superframe draws


# ------------------------------------------------------------------------------------------------ building streams
def superframes(seed, s, num_aus, pads, cuts=None):
    """pads: one item per access unit -- PAD bytes (carried in a data stream element), ("raw", bytes the body begins with),
    None (no PAD) or RANDOM; filled up with None to whole super-frames.  cuts: {super-frame: start addresses of AUs 1 ..},
    default evenly spaced.  -> (data [n][110 s], status [n]) as the follow call leaves them for clean reception."""
    rng = np.random.default_rng(seed)
    pads = list(pads) + [None] * (-len(pads) % num_aus)
    n_sf, size = len(pads) // num_aus, 110 * s
    data, status = np.zeros((n_sf, size), np.uint8), np.zeros(n_sf, P.STATUS_DTYPE)
    for k in range(n_sf):
        bodies = []
        for item in pads[k * num_aus:(k + 1) * num_aus]:
            bodies.append(NO_PAD if item is None else None if item is RANDOM else item[1] if isinstance(item, tuple) else synth.au_body(item))
        even = [FIRST[num_aus] + a * (size - FIRST[num_aus]) // num_aus for a in range(1, num_aus)]
        dac, sbr = KINDS[num_aus]
        sf, starts, _aus = synth.build_superframe(rng, 8 * s, dac_rate=dac, sbr=sbr, cuts=(cuts or {}).get(k, even), bodies=bodies)
        data[k] = sf[:size]
        status[k]["firecode_ok"], status[k]["num_aus"], status[k]["au_crc_mask"] = 1, num_aus, (1 << num_aus) - 1
        status[k]["au_start"][:num_aus + 1] = starts
    return data, status


def var(groups, index, **kw):
    return synth.dls_pads(groups, length_index=index, **kw)


def short(groups):
    return synth.dls_pads(groups)


def label(text, toggle=0, seg=16, charset=15):
    return synth.dls_segments(text, toggle, charset, seg)


class Scenario:
    def __init__(self, name, pads, text=None, charset=15, counts=None, damage=None, cuts=None):
        """text: the label after the scenario (None = whatever it was before, b"" = none); counts: counters of the scenario
        that the reference must report (a subset); damage(status rows of the scenario): reception losses"""
        self.name, self.pads, self.text, self.charset, self.counts, self.damage, self.cuts = name, pads, text, charset, counts or {}, damage, cuts


def clear_crc_bit(sf, a):
    def f(status):
        status[sf]["au_crc_mask"] &= ~(1 << a)
    return f


def firecode_fails(sf):
    def f(status):
        status[sf]["firecode_ok"], status[sf]["num_aus"], status[sf]["au_crc_mask"] = 0, 0, 0
    return f


def starts_out_of_range(status):
    status[0]["au_start"][1] = 99999              # AU 0 ends, AU 1 begins beyond the data part
    status[1]["au_start"][0] = -4                 # AU 0 begins before it
    status[1]["au_start"][1] = status[1]["au_start"][2] - 2        # AU 1 has no byte in front of its CRC


L128 = bytes(range(0x30, 0x30 + 64)) + bytes(range(0x41, 0x41 + 64))
UCS2 = "Ω→ラジオ".encode("utf-16-be")
IDX_TEXT = [b"index %d label" % i for i in range(8)]
BAD_CRC = bytearray(label(b"never shown")[0])
BAD_CRC[-1] ^= 0x40


def _streams():
    S = {}
    # A: s = 1, six access units of 14 bytes: short X-PAD only
    S["short"] = dict(s=1, num_aus=6, seed=11, scenarios=[
        Scenario("two-byte label: content indicator + one CI-less field", short(label(b"Hi")), b"Hi", counts=dict(groups_ok=1, aus_with_xpad=2, changes=1)),
        Scenario("a 20-byte group over six access units", short(label(b"sixteen bytes!!!")), b"sixteen bytes!!!",
                 counts=dict(groups_ok=1, aus_with_xpad=6, labels_completed=1)),
        Scenario("UCS-2, two segments", short(label(UCS2, 1, 8, 6)), UCS2, charset=6, counts=dict(groups_ok=2)),
    ])
    # B: s = 8, three access units: variable X-PAD at each of the eight length indices, one 14-byte label each
    S["indices"] = dict(s=8, num_aus=3, seed=12, scenarios=[
        Scenario("length index %d .. %d" % (i, i + 1), var(label(IDX_TEXT[i], i & 1), i) + var(label(IDX_TEXT[i + 1], ~i & 1), i + 1), IDX_TEXT[i + 1],
                 counts=dict(groups_ok=2, labels_completed=2, changes=2)) for i in (0, 2, 4, 6)])
    # C: s = 24, two access units: eight segments, one-byte segments, the escape byte
    S["segments"] = dict(s=24, num_aus=2, seed=13, scenarios=[
        Scenario("128 bytes in eight segments", var(label(L128), 5), L128, counts=dict(groups_ok=8, labels_completed=1)),
        Scenario("two one-byte segments", var(label(b"ab", 1, 1), 2), b"ab", counts=dict(groups_ok=2, labels_completed=1)),
        Scenario("PAD of 300 bytes: the escape byte", var(label(b"escaped", 0), 4, n=300) + var(label(b"just below", 1), 4, n=254), b"just below",
                 counts=dict(groups_ok=2, changes=2)),
    ])
    # D: s = 8, four access units: other applications beside the label, CI-less variable fields, the protocol
    x4, x8 = bytes([1, 2, 3, 4]), bytes(range(8))
    three, again = label(b"0123456789abcdefABCDEFGHIJKLMNOPxyz", 0), label(b"0123456789abcdefABCDEFGHIJKLMNOPxyz", 1)
    S["protocol"] = dict(s=8, num_aus=4, seed=14, scenarios=[
        Scenario("beside types 1, 12, 13 and an extended type; CI-less continuation",
                 var(label(b"with end marker", 0), 4, before=[(1, x4)], after=[(12, x8)]) +
                 var(label(b"four in the list", 1), 4, before=[(1, x4)], after=[(12, x8), (13, x4)]) +
                 var(label(b"behind type 31", 0), 4, before=[(31, 0x42, x8)]) +
                 var(label(b"CI-less fields", 1), 0, ci_less=True, before=[(13, x4)]), b"CI-less fields",
                 counts=dict(groups_ok=4, changes=4, aus_with_xpad=11, pad_malformed=0, fields_ignored=0)),
        Scenario("toggle change, then the label repeated", var(label(b"first", 0) + label(b"second", 1) + label(b"second", 1), 4), b"second",
                 counts=dict(labels_completed=3, changes=2)),
        Scenario("clear, DL Plus, an unknown command", var([synth.dls_command(1), synth.dls_command(2, 1, b"\x00\x01\x05\x09\x0a"), synth.dls_command(5)], 3), b"",
                 counts=dict(groups_ok=2, commands_ignored=2, changes=1, labels_completed=0)),
        Scenario("the middle segment never comes", var([three[0], three[2]], 5), b"", counts=dict(groups_ok=2, labels_completed=0)),
        Scenario("segments out of order, new toggle", var([again[2], again[0], again[1]], 5),
                 b"0123456789abcdefABCDEFGHIJKLMNOPxyz", counts=dict(groups_ok=3, labels_completed=1)),
    ])
    # E: s = 8, three access units: reception losses
    rep = var(label(b"from the repetition!"[:16]), 2)                # a 20-byte group in three sub-fields of 8
    S["loss"] = dict(s=8, num_aus=3, seed=15, scenarios=[
        Scenario("CRC bit cleared in the middle of a group", rep + rep, b"from the repetit", damage=clear_crc_bit(0, 1),
                 counts=dict(aus=6, aus_lost=1, groups_ok=1, groups_crc_failed=0, labels_completed=1)),
        Scenario("a super-frame whose Fire code fails", var(label(b"after the gap", 1), 4) + [None, None] + var(label(b"after the gap", 1), 4), b"after the gap",
                 damage=firecode_fails(0), counts=dict(aus=4, aus_lost=1, groups_ok=1)),
        Scenario("start addresses out of range", [None, None] + var(label(b"third unit", 0), 4) + [None, None] + var(label(b"sixth unit", 1), 4), b"sixth unit",
                 damage=starts_out_of_range, counts=dict(aus=6, aus_lost=4, groups_ok=2)),
    ])
    # F: s = 8, six access units: hand-made garbage, then what build_superframe draws
    V = lambda xpad, ci, n=None: synth.pad_field(bytes(xpad), 2, ci, n)
    hand = [("raw", bytes([0x80, 200]) + bytes(20)),                  # a count beyond the access unit
            ("raw", bytes([0x80, 255])),                              # the escape, and the access unit ends (len == 2)
            ("raw", bytes([0x80, 0])), ("raw", bytes([0x80, 1, 0x20])),                       # n = 0, n = 1
            V([(7 << 5) | 2], 1, 7),                                  # one sub-field of 48 bytes in a field of 5
            V([(0 << 5) | 2, (0 << 5) | 3], 1),                       # the list runs into the end of the field
            V([31], 1),                                               # type 31 as the last byte
            V([9, 9, 9, 9], 0),                                       # a CI-less variable field on a fresh state
            synth.pad_field(bytes(4), 1, 0),                          # ... and a short one
            synth.pad_field(bytes(3), 1, 1),                          # short X-PAD of three bytes
            ] + var([bytes(BAD_CRC)], 4) + var(label(b"still works"), 4)
    S["garbage"] = dict(s=8, num_aus=6, seed=16, scenarios=[
        Scenario("hand-made", hand, b"still works", cuts={0: [11 + 140, 11 + 144, 11 + 290, 11 + 430, 11 + 570]},
                 counts=dict(pad_malformed=8, fields_ignored=2, groups_crc_failed=1, groups_ok=1)),
        Scenario("random bodies", [RANDOM] * 60),
    ])
    S["random"] = dict(s=24, num_aus=6, seed=17, scenarios=[Scenario("random bodies", [RANDOM] * 72)])
    # H: the chunking stream: 12 super-frames of three access units, groups that cross every boundary
    groups = (label(b"one segment", 0) + label(b"two segments, twenty-six", 1) + [synth.dls_command(2, 1, b"\x00\x01\x02")] +
              label(b"0123456789abcdefABCDEFGHIJKLMNOPxyz", 0) + label(b"thirty-two bytes in two segments", 1) + [synth.dls_command(1)] + label(b"the last one of them", 1))
    pads = var(groups, 1, ci_less=True)
    assert len(pads) == 36
    S["chunks"] = dict(s=8, num_aus=3, seed=18, scenarios=[Scenario("twelve super-frames", pads, b"the last one of them")])
    return S


STREAMS = _streams()
#: what follows the chunking stream: a group begun in its own first access unit and ended CI-less -- and one that relies on
#: a context the stream does not leave
NEXT_CALL = var(label(b"and the next call", 0), 2, ci_less=True)


@pytest.fixture(scope="module")
def built_streams(built):
    """name -> dict(s, data, status, bounds: [(scenario, first super-frame, end)])"""
    out = {}
    for name, spec in STREAMS.items():
        datas, stats, bounds, at = [], [], [], 0
        for k, sc in enumerate(spec["scenarios"]):
            d, st = superframes(spec["seed"] * 100 + k, spec["s"], spec["num_aus"], sc.pads, sc.cuts)
            if sc.damage:
                sc.damage(st)
            datas.append(d); stats.append(st)
            bounds.append((sc, at, at + len(d)))
            at += len(d)
        out[name] = dict(s=spec["s"], data=np.concatenate(datas), status=np.concatenate(stats), bounds=bounds)
        assert at <= 12, (name, at)
    return out


# ------------------------------------------------------------------------------------------------ one call, on any memory
class HostMemory:
    def load(self, image):
        raw = np.empty(image.size + 256, np.uint8)
        off = -raw.ctypes.data % 256
        self.buf = raw[off:off + image.size]
        self.buf[:] = image
        return self.buf.ctypes.data

    def run(self, entries):
        dabgpu.pad_labels_host(entries)

    def read(self):
        return self.buf.copy()


class DeviceMemory:
    def __init__(self, ctx):
        self.ctx = ctx

    def load(self, image):
        import torch
        self.t = torch.from_numpy(image).cuda()
        return self.t.data_ptr()

    def run(self, entries):
        self.ctx.pad_labels_dev(entries)
        self.ctx.sync()

    def read(self):
        self.ctx.sync()
        return self.t.cpu().numpy()


def call(mem, specs, mutate=None, refused=False):
    """One call on buffers laid out in one allocation, every region between sentinel bytes.  specs: dicts {s, data [rows][110 s],
    status [rows], n (what d_follow says), max_sf (default: the rows), state (bytes or None = NULL), stride, data_off (the
    data rows begin that many bytes, below 16, off their 256-byte boundary)}.  After the call
    nothing but the state-out, label and result regions may have changed (none at all for a refused call).
    -> per entry (label record, result record, state bytes)"""
    size, lay = 0, []

    def take(n):
        nonlocal size
        off = (size + GAP + 255) // 256 * 256
        size = off + n
        return off

    nb = dabgpu.pad_state_bytes()
    for sp in specs:
        rows, stride = len(sp["data"]), sp.get("stride", 110 * sp["s"])
        assert 0 <= sp.get("data_off", 0) < 16
        lay.append(dict(data=take(max(rows, 1) * stride + 16) + sp.get("data_off", 0), status=take(max(rows, 1) * 64), follow=take(32),
                        sin=take(nb) if sp.get("state") is not None else None, sout=take(nb), label=take(144), result=take(64)))
    image = np.full(size + GAP, FILL, np.uint8)
    for sp, L in zip(specs, lay):
        stride = sp.get("stride", 110 * sp["s"])
        for k, row in enumerate(sp["data"]):
            image[L["data"] + k * stride:L["data"] + k * stride + row.size] = row
        image[L["status"]:L["status"] + 64 * len(sp["data"])] = np.asarray(sp["status"]).view(np.uint8).reshape(-1)
        fr = np.zeros(1, dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)
        fr["n_superframes"], fr["phase"], fr["synced"] = sp["n"], 0, 1
        image[L["follow"]:L["follow"] + 32] = fr.view(np.uint8)
        if L["sin"] is not None:
            image[L["sin"]:L["sin"] + nb] = np.frombuffer(bytes(sp["state"]), np.uint8)
    base = mem.load(image)
    assert base % 256 == 0
    entries = [dabgpu.PadEntry(base + L["data"], sp.get("stride", 110 * sp["s"]), base + L["status"], base + L["follow"], 8 * sp["s"],
                               sp.get("max_sf", len(sp["data"])), base + L["sin"] if L["sin"] is not None else None, base + L["sout"],
                               base + L["label"], base + L["result"]) for sp, L in zip(specs, lay)]
    if mutate:
        mutate(entries)
    if refused:
        with pytest.raises(dabgpu.DabGpuError) as err:
            mem.run(entries)
        assert err.value.status == ARG
        assert (mem.read() == image).all(), "a refused call wrote"
        return None
    mem.run(entries)
    after = mem.read()
    out, untouched = [], np.ones(after.size, bool)
    for L in lay:
        for key, n in (("sout", nb), ("label", 144), ("result", 64)):
            untouched[L[key]:L[key] + n] = False
        out.append((after[L["label"]:L["label"] + 144].copy().view(dabgpu.PAD_LABEL_DTYPE), after[L["result"]:L["result"] + 64].copy().view(dabgpu.PAD_RESULT_DTYPE),
                    after[L["sout"]:L["sout"] + nb].copy()))
    assert (after[untouched] == image[untouched]).all(), "bytes outside the outputs changed"
    return out


def same(got, want):
    """(label, result) records: byte for byte"""
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def explain(got, want):
    return "\n got  %s %s\n want %s %s" % (got[0], got[1], want[0], want[1])


def text_of(rec):
    return bytes(rec["text"][0][:int(rec["length"][0])])


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_records_and_sizes(built, tmp_path):
    L = dabgpu.lib()
    for name in ("dabgpu_pad_state_bytes", "dabgpu_pad_labels_dev", "dabgpu_pad_labels_host", "dabgpu_pad_label_utf8"):
        assert name in dabgpu.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.dabgpu_abi_version() == 6 == dabgpu.ABI_VERSION
    assert dabgpu.PAD_LABEL_DTYPE.itemsize == 144 == P.LABEL_DTYPE.itemsize and dabgpu.PAD_LABEL_DTYPE.names == P.LABEL_DTYPE.names
    assert dabgpu.PAD_RESULT_DTYPE.itemsize == 64 == P.RESULT_DTYPE.itemsize and dabgpu.PAD_RESULT_DTYPE.names == P.RESULT_DTYPE.names
    assert dabgpu.pad_state_bytes() % 16 == 0 and dabgpu.pad_state_bytes() >= 144 + 8 * 17 + 20
    assert hasattr(dabgpu.Context, "pad_labels_dev")
    # the binding's structure and the records against the header, as the C compiler lays them out
    fields = [f for f, _ in dabgpu.PadEntry._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dabgpu.h"\nint main(void) {\n' +
                   '  printf("%zu %zu %zu", sizeof(dabgpu_pad_entry), sizeof(dabgpu_pad_label), sizeof(dabgpu_pad_result));\n' +
                   "".join('  printf(" %%zu", offsetof(dabgpu_pad_entry, %s));\n' % f for f in fields) +
                   "".join('  printf(" %%zu", offsetof(dabgpu_pad_label, %s));\n' % f for f in dabgpu.PAD_LABEL_DTYPE.names) +
                   "".join('  printf(" %%zu", offsetof(dabgpu_pad_result, %s));\n' % f for f in dabgpu.PAD_RESULT_DTYPE.names) +
                   '  return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(dabgpu.PadEntry), 144, 64] + [getattr(dabgpu.PadEntry, f).offset for f in fields]
    want += [dabgpu.PAD_LABEL_DTYPE.fields[f][1] for f in dabgpu.PAD_LABEL_DTYPE.names]
    want += [dabgpu.PAD_RESULT_DTYPE.fields[f][1] for f in dabgpu.PAD_RESULT_DTYPE.names]
    assert got == want


def spoil(field, value, at=-1):
    def f(entries):
        setattr(entries[at], field, value(entries[at]) if callable(value) else value)
    return f


#: each refused with DABGPU_ERR_ARG, the bad entry LAST in the table: nothing of the good ones before it is written
BAD_ENTRIES = [spoil("bitrate_kbps", 12), spoil("bitrate_kbps", 0), spoil("bitrate_kbps", 520), spoil("data_stride", 879),
               spoil("max_superframes", -1), spoil("d_data", None), spoil("d_status", None), spoil("d_follow", None),
               spoil("d_state_out", None), spoil("d_label", None), spoil("d_result", None),
               spoil("d_state_in", lambda e: e.d_state_in + 8), spoil("d_state_out", lambda e: e.d_state_out + 4),
               spoil("d_state_out", lambda e: e.d_state_in), spoil("d_state_out", lambda e: e.d_state_in + 16),
               spoil("d_state_out", lambda e: e.d_state_in - 16),
               spoil("d_label", lambda e: e.d_label + 2), spoil("d_result", lambda e: e.d_result + 1),
               spoil("d_status", lambda e: e.d_status + 2), spoil("d_follow", lambda e: e.d_follow + 2)]


def refusal_specs(built_streams):
    st = built_streams["protocol"]
    zero = np.zeros(dabgpu.pad_state_bytes(), np.uint8)
    return [dict(s=8, data=st["data"][:2], status=st["status"][:2], n=2, state=zero) for _ in range(3)]


def test_refusals_that_need_no_device(built_streams):
    L = dabgpu.lib()
    specs = refusal_specs(built_streams)
    for m in BAD_ENTRIES:
        call(HostMemory(), specs, mutate=m, refused=True)
    good = (dabgpu.PadEntry * 1)(dabgpu.PadEntry(0x10000, 880, 0x20000, 0x30000, 64, 2, None, 0x40000, 0x50000, 0x60000))
    assert L.dabgpu_pad_labels_host(None, 1) == ARG and L.dabgpu_pad_labels_host(good, -1) == ARG
    assert L.dabgpu_pad_labels_host(None, 0) == 0
    # the device call checks the same table before it looks for a device: no context, then the table
    assert L.dabgpu_pad_labels_dev(None, good, 1, None) == ARG
    got = call(HostMemory(), specs)                                  # ... and the unspoilt table goes through
    assert all(int(r[1]["aus"][0]) == 8 for r in got)


@pytest.mark.parametrize("name", list(STREAMS))
def test_host_equals_the_reference_scenario_by_scenario(built_streams, name):
    """one call per scenario, the state handed on: label and counters equal the reference's; the reference itself reports
    what the scenario is about, and the label that was sent"""
    st = built_streams[name]
    rx, state = P.Receiver(), None
    for sc, a, b in st["bounds"]:
        want = rx.call(st["data"][a:b], st["status"][a:b], b - a, st["s"])
        got = call(HostMemory(), [dict(s=st["s"], data=st["data"][a:b], status=st["status"][a:b], n=b - a, state=state)])[0]
        assert same(got, want), sc.name + explain(got, want)
        state = got[2]
        if sc.text is not None:
            assert text_of(want[0]) == sc.text, (sc.name, text_of(want[0]))
            assert int(want[0]["charset"][0]) == (sc.charset if sc.text else 0)
        for key, value in sc.counts.items():
            assert int(want[1][key][0]) == value, (sc.name, key, want[1])


def test_round_trip_covers_what_it_should(built_streams):
    """segments 1, 2, 8; 1-byte and 16-byte segments; s = 1, 8, 24 with 2, 3, 4, 6 access units; both element forms; every index"""
    assert {(v["s"], v["num_aus"]) for v in STREAMS.values()} >= {(1, 6), (8, 3), (24, 2), (8, 4), (8, 6), (24, 6)}
    assert len(label(L128)) == 8 and all(len(g) == 20 for g in label(L128)) and len(label(b"ab", 0, 1)) == 2 and len(label(b"Hi")) == 1
    assert len(short(label(b"sixteen bytes!!!"))) == 6
    assert synth.dse(bytes(300))[1:3] == bytes([255, 45]) and synth.dse(bytes(254))[1] == 254 and len(synth.dse(bytes(254))) == 256
    assert synth.xpad_variable([(2, bytes(4))])[1] == 0 and len(synth.xpad_variable([(2, bytes(4))] * 4)) == 20
    with pytest.raises(AssertionError):
        synth.dse(bytes(300), escape=False)
    # build_superframe without bodies draws what it always drew
    a = synth.build_superframe(np.random.default_rng(5), 64, 1, 1)
    b = synth.build_superframe(np.random.default_rng(5), 64, 1, 1, bodies=[None, NO_PAD, None])
    assert (a[0][:880] != b[0][:880]).sum() <= 3 and a[1] == b[1]
    assert (a[2][0] == b[2][0]).all() and (a[2][2] == b[2][2]).all() and (a[2][1][1:-2] == b[2][1][1:-2]).all()


def test_garbage_minima_then_equality(built_streams):
    """the seeds were picked so that the reference alone reports, over the garbage streams, every kind of trouble; then the
    host call equals it (whole streams, one call each)"""
    totals, dse_first = dict.fromkeys(P.COUNTERS, 0), 0
    for name in ("garbage", "random"):
        st = built_streams[name]
        n = len(st["data"])
        want = P.Receiver().call(st["data"], st["status"], n, st["s"])
        for k in P.COUNTERS:
            totals[k] += int(want[1][k][0])
        for row, s in zip(st["data"], st["status"]):
            dse_first += sum(1 for a in range(s["num_aus"]) if s["au_start"][a + 1] - s["au_start"][a] - 2 >= 1 and row[s["au_start"][a]] >> 5 == 4)
        got = call(HostMemory(), [dict(s=st["s"], data=st["data"], status=st["status"], n=n)])[0]
        assert same(got, want), name + explain(got, want)
    assert totals["pad_malformed"] >= 1 and totals["fields_ignored"] >= 1 and totals["groups_crc_failed"] >= 1 and dse_first >= 20, (totals, dse_first)


CHUNKINGS = [[12], [1] * 12, [5, 7], [0, 3, 9]]


def chunked(mem_of, st, chunks, swap=False):
    """the chunking stream in calls of `chunks` super-frames, then NEXT_CALL -> (labels and results per call, last state).
    swap: two state records, swapped call to call, on one allocation (the device test)"""
    nxt = superframes(99, st["s"], 3, NEXT_CALL)
    state, at, out = None, 0, []
    for n in list(chunks) + ["next"]:
        if n == "next":
            data, status, n = nxt[0], nxt[1], len(nxt[0])
        else:
            data, status = st["data"][at:at + n], st["status"][at:at + n]
            at += n
        # a chunk of no super-frames keeps its row: d_follow says 0
        rows = (data, status) if n else (st["data"][:1], st["status"][:1])
        r = call(mem_of(), [dict(s=st["s"], data=rows[0], status=rows[1], n=n, state=state)])[0]
        out.append(r)
        state = r[2]
    return out, state


def check_chunkings(mem_of, st):
    whole = P.Receiver()
    want = [whole.call(st["data"], st["status"], 12, st["s"])]
    nxt = superframes(99, st["s"], 3, NEXT_CALL)
    want.append(whole.call(nxt[0], nxt[1], len(nxt[0]), st["s"]))
    assert text_of(want[0][0]) == b"the last one of them" and text_of(want[1][0]) == b"and the next call"
    states = []
    for chunks in CHUNKINGS:
        got, state = chunked(mem_of, st, chunks)
        ref = P.run_chunks(st["data"], st["status"], st["s"], chunks)
        for g, w in zip(got[:-1], ref):
            assert same(g, w), (chunks, explain(g, w))
        assert got[-2][0].tobytes() == want[0][0].tobytes(), chunks                   # the final label
        assert P.total([g[1] for g in got[:-1]]) == P.total([want[0][1]]), chunks      # the summed counters
        assert same(got[-1], want[1]), (chunks, explain(got[-1], want[1]))            # the next call
        states.append(state.tobytes())
    assert len(set(states)) == 1
    return states[0]


def test_chunkings_agree(built_streams):
    check_chunkings(HostMemory, built_streams["chunks"])


def rec(text, charset):
    r = np.zeros(1, dabgpu.PAD_LABEL_DTYPE)
    r["length"], r["charset"] = len(text), charset
    r["text"][0, :len(text)] = np.frombuffer(bytes(text), np.uint8)
    return r


def test_label_as_utf8(built):
    L = dabgpu.lib()
    for s in ("plain", "Grüße, Ω→ラジオ 🎵", "", "x" * 128):
        assert dabgpu.pad_label_utf8(rec(s.encode("utf-8"), 15)) == s
    bad = [b"\x80", b"ab\xc3", b"\xc3\x28", b"\xc0\xaf", b"\xe0\x80\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xf8\x88\x80\x80\x80", b"a\x00b",
           b"\xe2\x82", b"\xf0\x9f\x8e"]
    for raw in bad:
        with pytest.raises(dabgpu.DabGpuError) as err:
            dabgpu.pad_label_utf8(rec(raw, 15))
        assert err.value.status == ARG, raw
    bmp = "Ω→ラジオ ÿĀ߿ࠀ￿"                                       # every UTF-8 length a BMP character can have, no surrogate
    assert dabgpu.pad_label_utf8(rec(bmp.encode("utf-16-be"), 6)) == bmp
    for raw in (b"\x00", b"\xd8\x00\xdc\x00", b"\xdc\x00", b"\x00\x00"):
        with pytest.raises(dabgpu.DabGpuError) as err:
            dabgpu.pad_label_utf8(rec(raw, 6))
        assert err.value.status == ARG, raw
    for charset in (0, 1, 4, 5, 7, 14):
        with pytest.raises(dabgpu.DabGpuError) as err:
            dabgpu.pad_label_utf8(rec(b"abc", charset))
        assert err.value.status == PROFILE
    r = rec(b"abcdef", 15)
    buf = C.create_string_buffer(b"\x55" * 16, 16)
    assert L.dabgpu_pad_label_utf8(r.ctypes.data, buf, 6) == CAPACITY and buf.raw == b"\x55" * 16       # no room for the NUL
    assert L.dabgpu_pad_label_utf8(r.ctypes.data, buf, 7) == 6 and buf.raw == b"abcdef\x00" + b"\x55" * 9
    assert L.dabgpu_pad_label_utf8(r.ctypes.data, buf, 0) == ARG and L.dabgpu_pad_label_utf8(None, buf, 7) == ARG
    assert L.dabgpu_pad_label_utf8(r.ctypes.data, None, 7) == ARG
    r["length"] = 129
    assert L.dabgpu_pad_label_utf8(r.ctypes.data, buf, 16) == ARG


def test_new_kernel_neither_spills_nor_uses_scratch(built, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the device assembly cannot be checked")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    out = tmp_path / "pad_kernels.s"
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "pad_kernels.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    md = kernel_metadata(out.read_text())
    kernels = [v for k, v in md.items() if "pad_labels_kernel" in k]
    assert len(kernels) == 1 and len(md) == 1
    v = kernels[0]
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v


def test_walk_fuzz_under_sanitizers(tmp_path):
    """tests/pad_walk_fuzz.cpp: 200 000 walks over random and mutated-valid access units, each at the end of an exactly
    sized heap block, built with the host compiler under AddressSanitizer and UBSan and run as a child process"""
    exe = str(tmp_path / "pad_walk_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pad_walk_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "200000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "walks=200000" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = dict(kv.split("=") for kv in r.stdout.split())
    assert int(got["labels"]) > 0 and int(got["malformed"]) > 0 and int(got["lost"]) > 0, r.stdout


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.gpu
def test_gpu_every_case_in_one_ragged_call(pctx, built_streams):
    """the eight streams in ONE call: bit rates 8, 64 and 192, n_superframes read from the device's follow records (all
    different from the rows that exist), two rows of 0xFF behind every stream, one entry whose max_superframes is smaller
    than what its follow record says: label, counters and state record equal the reference and the host call"""
    names = list(STREAMS)
    assert len(names) == 8
    specs, wants = [], []
    for e, name in enumerate(names):
        st = built_streams[name]
        n = len(st["data"])
        ff = np.full((2, 110 * st["s"]), 0xFF, np.uint8)
        ffs = np.full(2 * 64, 0xFF, np.uint8).view(P.STATUS_DTYPE)
        sp = dict(s=st["s"], data=np.concatenate([st["data"], ff]), status=np.concatenate([st["status"], ffs]), n=n,
                  stride=110 * st["s"] + [0, 2, 16][e % 3])
        used = n
        if name == "random":
            sp["n"], sp["max_sf"], used = 40, 7, 7                    # the follow record says more than there are rows
            sp["data"], sp["status"] = sp["data"][:7], sp["status"][:7]
        specs.append(sp)
        wants.append(P.Receiver().call(st["data"], st["status"], used, st["s"]))
    assert {sp["s"] for sp in specs} == {1, 8, 24} and len({sp["n"] for sp in specs}) >= 4
    got = call(DeviceMemory(pctx), specs)
    host = call(HostMemory(), specs)
    for name, g, h, w in zip(names, got, host, wants):
        assert same(g, w), name + explain(g, w)
        assert same(h, w) and g[2].tobytes() == h[2].tobytes(), name
    assert [text_of(g[0]) for g in got[:5]] == [UCS2, IDX_TEXT[7], b"just below", b"0123456789abcdefABCDEFGHIJKLMNOPxyz", b"sixth unit"]
    # rows beyond n_superframes: read them (n + 2) and the 0xFF rows count -- that they changed nothing above was no accident
    more = dict(specs[0], n=specs[0]["n"] + 2)
    assert int(call(DeviceMemory(pctx), [more])[0][1]["aus"][0]) > int(got[0][1]["aus"][0])


@pytest.mark.gpu
def test_gpu_chunkings_agree_with_the_state_handed_on(pctx, built_streams):
    state = check_chunkings(lambda: DeviceMemory(pctx), built_streams["chunks"])
    assert state == check_chunkings(HostMemory, built_streams["chunks"])


@pytest.mark.gpu
def test_gpu_state_records_swap_call_to_call(pctx, built_streams):
    """two state records on the device, swapped call to call as a receiver keeps them; labels and results of every call
    stay on the device until the end"""
    import torch
    st = built_streams["chunks"]
    s, nb = st["s"], dabgpu.pad_state_bytes()
    data = torch.from_numpy(st["data"]).cuda()
    status = torch.from_numpy(st["status"].view(np.uint8).reshape(12, 64).copy()).cuda()
    follow = np.zeros(4, dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)
    follow["n_superframes"] = [5, 0, 4, 3]
    d_follow = torch.from_numpy(follow.view(np.uint8).reshape(4, 32).copy()).cuda()
    states = torch.zeros((2, nb), dtype=torch.uint8, device="cuda")
    labels = torch.zeros((4, 144), dtype=torch.uint8, device="cuda")
    results = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    at = 0
    for k, n in enumerate([5, 0, 4, 3]):
        row = min(at, 11)
        pctx.pad_labels_dev([dabgpu.PadEntry(data[row].data_ptr(), 110 * s, status[row].data_ptr(), d_follow[k].data_ptr(), 8 * s, 12 - row,
                                             states[k & 1].data_ptr(), states[~k & 1].data_ptr(), labels[k].data_ptr(), results[k].data_ptr())])
        at += n
    pctx.sync()
    want = P.run_chunks(st["data"], st["status"], s, [5, 0, 4, 3])
    got_l, got_r = labels.cpu().numpy(), results.cpu().numpy()
    for k in range(4):
        assert got_l[k].tobytes() == want[k][0].tobytes() and got_r[k].tobytes() == want[k][1].tobytes(), k
    assert text_of(want[3][0]) == b"the last one of them"


@pytest.mark.gpu
def test_gpu_refused_calls_leave_every_output_alone(pctx, built_streams):
    specs = refusal_specs(built_streams)
    for m in BAD_ENTRIES:
        call(DeviceMemory(pctx), specs, mutate=m, refused=True)
    with pytest.raises(dabgpu.DabGpuError):
        pctx.pad_labels_dev([dabgpu.PadEntry()], None)
    pctx.pad_labels_dev([])                                          # nothing to do is not an error
    got = call(DeviceMemory(pctx), specs)
    assert all(int(r[1]["aus"][0]) == 8 for r in got)


# ---- end to end
E2E_SERVICES = [("Radio One", 0xC221, 3, 0, 3, 64, 0), ("Jazz 24", 0xC222, 7, 0, 2, 48, 48)]
E2E_LABELS = ["Now: Ω Quartet – Blue in Green".encode("utf-8"), "Nachrichten um 12".encode("utf-8")]
E2E_SEED = 4                                                          # (every access unit has room for its PAD element)


def e2e_bodies():
    """twelve access units per service and cycle: service 0 sends its label in two sub-fields of 24 bytes (twice), service 1
    in short X-PAD, six access units a time"""
    first = var(label(E2E_LABELS[0], 1), 5)
    first = (first + [None] * 4) * 2
    second = short(label(E2E_LABELS[1], 0, 16)[:1]) + short(label(E2E_LABELS[1], 0, 16)[1:]) + [None] * 6
    second = (second + [None] * 12)[:12]
    cut = lambda pads: [[synth.au_body(p) if p is not None else NO_PAD for p in pads[3 * q:3 * q + 3]] for q in range(4)]
    return [cut(first), cut(second)]


def test_end_to_end_multiplex_carries_both_labels(built):
    """what the GPU test will receive, through the reference receiver on the transmitted super-frames"""
    ens = synth.ServiceEnsemble(E2E_SEED, E2E_SERVICES, n_frames=5, extras=False, bodies=e2e_bodies())
    for n, (svc, sent) in enumerate(zip(E2E_SERVICES, E2E_LABELS)):
        s = svc[5] // 8
        data = np.stack([sf[:110 * s] for sf in ens.superframes[n]])
        status = np.zeros(4, P.STATUS_DTYPE)
        status["firecode_ok"], status["num_aus"], status["au_crc_mask"] = 1, 3, 7
        for q in range(4):
            status[q]["au_start"][:4] = [6] + [6 + sum(len(a) for a in ens.aus[n][q][:k + 1]) for k in range(3)]
        lab, res = P.Receiver().call(data, status, 4, s)
        assert text_of(lab) == sent and int(res["pad_malformed"][0]) == 0, (n, res)


@pytest.mark.gpu
def test_gpu_end_to_end_iq_to_labels(pctx):
    """IQ of a multiplex whose two DAB+ services carry two labels -> front end -> FIC pass -> decode_ensembles_dev ->
    dabplus_follow_dev -> pad_labels_dev on the same stream, three calls of 16 frames, the records swapped: both labels"""
    import torch
    dev = torch.device("cuda", 0)
    fps, n_calls, L, FB = 16, 3, 76 * 2552, dabgpu.NB_FRAME_BITS
    ens = synth.ServiceEnsemble(E2E_SEED, E2E_SERVICES, n_frames=5, extras=False, bodies=e2e_bodies())
    tx = ens.iq()
    rng = np.random.default_rng(12)
    c = pctx
    c.streams_reset(1)
    plans = None
    n_cifs, max_sf, nb = 4 * fps, (4 * fps + 4) // 5, dabgpu.pad_state_bytes()
    labels = torch.zeros((2, 144), dtype=torch.uint8, device=dev)
    results = torch.zeros((n_calls, 2, 64), dtype=torch.uint8, device=dev)
    for call_no in range(n_calls):
        idx = (np.arange(fps) + call_no * fps) % 5
        rx = synth.channel(tx[idx].ravel(), snr_db=20.0, rng=rng).reshape(fps, -1)
        d_iq = torch.from_numpy(np.ascontiguousarray(rx[:, synth.NB_NULL:synth.NB_NULL + L]).astype(np.complex64)).to(dev)
        d_soft = torch.zeros((fps, FB), dtype=torch.int8, device=dev)
        c.ofdm_demod_streams_dev(d_iq.data_ptr(), L, 1, fps, 0.9, d_soft.data_ptr(), None, None)
        fib = torch.zeros((fps, 12, 32), dtype=torch.uint8, device=dev)
        ok = torch.zeros((fps, 12), dtype=torch.uint8, device=dev)
        if plans is None:
            c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), [[]], None, None, None, None)
            c.sync()
            fib_h, ok_h = fib.cpu().numpy(), ok.cpu().numpy()
            assert ok_h.all()
            plans = [dabgpu.fig_subchannels(fib_h, ok_h)]
            comps = dabgpu.fig_audio_components(fib_h, ok_h)
            assert [cp.ascty for cp in comps] == [63, 63] and [sc.bitrate_kbps for sc in plans[0]] == [64, 48]
            hist = [[[torch.zeros((15, sc.length * 64), dtype=torch.int8, device=dev) for sc in plans[0]]] for _ in range(2)]
            carry = [[torch.zeros(dabgpu.dabplus_carry_bytes(sc.bitrate_kbps), dtype=torch.uint8, device=dev) for sc in plans[0]] for _ in range(2)]
            state = [[torch.zeros(nb, dtype=torch.uint8, device=dev) for _sc in plans[0]] for _ in range(2)]
        outs = [[torch.zeros((n_cifs, sc.bitrate_kbps * 3), dtype=torch.uint8, device=dev) for sc in plans[0]]]
        ptrs = lambda lsts: [[x.data_ptr() for x in lst] for lst in lsts]
        c.decode_ensembles_dev(d_soft.data_ptr(), FB, 1, fps, fib.data_ptr(), ok.data_ptr(), plans, ptrs(hist[0]) if call_no else None,
                               ptrs(hist[1]), ptrs(outs), None)
        follow, pads, keep = [], [], []
        for j, sc in enumerate(plans[0]):
            br = sc.bitrate_kbps
            data = torch.zeros((max_sf, 110 * br // 8), dtype=torch.uint8, device=dev)
            st = torch.zeros((max_sf * 64,), dtype=torch.uint8, device=dev)
            res = torch.zeros((32,), dtype=torch.uint8, device=dev)
            keep.append((data, st, res))
            follow.append(dabgpu.DabplusEntry(outs[0][j].data_ptr(), 3 * br, br, carry[0][j].data_ptr() if call_no else None, carry[1][j].data_ptr(),
                                              data.data_ptr(), st.data_ptr(), res.data_ptr()))
            pads.append(dabgpu.PadEntry(data.data_ptr(), 110 * br // 8, st.data_ptr(), res.data_ptr(), br, max_sf,
                                        state[0][j].data_ptr() if call_no else None, state[1][j].data_ptr(), labels[j].data_ptr(),
                                        results[call_no, j].data_ptr()))
        c.dabplus_follow_dev(follow, n_cifs)
        c.pad_labels_dev(pads)                                       # behind it on the same stream: nothing waits in between
        c.sync()
        for lst in (hist, carry, state):
            lst.reverse()
    got = labels.cpu().numpy().view(dabgpu.PAD_LABEL_DTYPE).reshape(2)
    counts = results.cpu().numpy().view(dabgpu.PAD_RESULT_DTYPE).reshape(n_calls, 2)
    for j in range(2):
        assert dabgpu.pad_label_utf8(got[j]) == E2E_LABELS[j].decode("utf-8"), (j, counts[:, j])
        assert got[j]["charset"] == 15 and got[j]["toggle"] == 1 - j
        assert counts[:, j]["labels_completed"].sum() >= 4 and counts[:, j]["changes"].sum() == 1 and counts[:, j]["groups_crc_failed"].sum() == 0
