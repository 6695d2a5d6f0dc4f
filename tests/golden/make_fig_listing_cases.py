"""Records what the five FIG listing calls of the C ABI (dabgpu_fig_subchannels, _audio_components, _packet_components,
_user_applications, _stream_components) return on seeded FIB batches -> fig_listing_cases.npz, which tests/test_fig_listings.py
holds every later library to, byte for byte.  Run against the library the recording is to stand for:

    python tests/golden/make_fig_listing_cases.py

The batches are ensembles from the synth.fig0* builders and synth._bits, then damaged in their structure (FIGs cut by a byte and by
a field, header flags flipped, reserved and invalid protection, duplicates, counts larger than the body, end markers and zero
lengths mid-FIB, failed CRCs, more entries than a call keeps).  Every call runs at three sizes of its output -- large, exactly
what it found, one too small -- into a buffer of max + 1 entries filled with FILL, so what a call leaves alone is recorded too."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import ctypes as C  # noqa: E402

import dabgpu  # noqa: E402
from dabgpu import synth  # noqa: E402
from dabgpu.synth import _bits, fig0  # noqa: E402

PATH = os.path.join(HERE, "fig_listing_cases.npz")
FILL = 0xA5
N_FILL = -7777                      # *n before the call
MAX_LARGE = 320
#: call -> bytes of one output entry
CALLS = {"subchannels": 24, "audio_components": 32, "packet_components": 48, "user_applications": 56, "stream_components": 32}
OK, ERR_PROFILE, ERR_CAPACITY = 0, -5, -6       # dabgpu_status (include/dabgpu.h)


def run_call(call, fib, crc_ok, max_out):
    """One call on fib [n_frames * 12][32], crc_ok [n_frames * 12] -> (status, *n, the max_out + 1 entries of the buffer)."""
    fib = np.ascontiguousarray(fib, np.uint8)
    crc_ok = np.ascontiguousarray(crc_ok, np.uint8)
    out = np.full((max_out + 1) * CALLS[call], FILL, np.uint8)
    n = C.c_int(N_FILL)
    fn = getattr(dabgpu.lib(), "dabgpu_fig_" + call)
    # (an empty batch still passes addresses: the calls refuse NULL)
    rc = fn(dabgpu._p(fib) if fib.size else dabgpu._p(np.zeros(1, np.uint8)), dabgpu._p(crc_ok) if crc_ok.size else dabgpu._p(np.zeros(1, np.uint8)),
            crc_ok.size // 12, dabgpu._p(out), max_out, C.byref(n))
    return int(rc), int(n.value), out


def three_sizes(call, fib, crc_ok):
    """[(max, status, n, buffer)] at max large, exact and one too small (a call that found nothing, or refused: 0 and 0)."""
    rows = [(MAX_LARGE,) + run_call(call, fib, crc_ok, MAX_LARGE)]
    found = rows[0][2] if rows[0][2] >= 0 else 0
    for m in (found, max(found - 1, 0)):
        rows.append((m,) + run_call(call, fib, crc_ok, m))
    return rows


# ------------------------------------------------------------------ FIGs the synth builders do not make
def fig0_2_mixed(services, pd=0):
    """services: (sid, [component]) with component = ("audio", ascty, subchid, primary) | ("stream", dscty, subchid, primary, ca) |
    ("packet", scid, primary) | ("fidc", dscty, fidcid)"""
    body = b""
    for sid, comps in services:
        body += _bits((sid, 32 if pd else 16), (0, 1), (0, 3), (len(comps), 4))
        for c in comps:
            if c[0] == "audio":
                body += _bits((0, 2), (c[1], 6), (c[2], 6), (c[3], 1), (0, 1))
            elif c[0] == "stream":
                body += _bits((1, 2), (c[1], 6), (c[2], 6), (c[3], 1), (c[4], 1))
            elif c[0] == "fidc":
                body += _bits((2, 2), (c[1], 6), (c[2], 6), (1, 1), (0, 1))
            else:
                body += _bits((3, 2), (c[1], 12), (c[2], 1), (0, 1))
    return fig0(2, body, pd=pd)


def fig0_8_any(entries, pd=0):
    """entries: (sid, scids, form, id, extended) with form "short" (SubChId), "fidc" (short, MSC/FIC flag 1) or "long" (SCId)"""
    body = b""
    for sid, scids, form, ident, extended in entries:
        body += _bits((sid, 32 if pd else 16), (extended, 1), (0, 3), (scids, 4))
        if form == "long":
            body += _bits((1, 1), (0, 3), (ident, 12))
        else:
            body += _bits((0, 1), (1 if form == "fidc" else 0, 1), (ident, 6))
        if extended:
            body += b"\x00"
    return fig0(8, body, pd=pd)


def refig(fig, body):
    """the FIG with another body (the FIG 0 header byte kept)"""
    data = fig[1:2] + body
    return _bits((0, 3), (len(data), 5)) + data


def cut(fig, n):
    """the FIG with its last n bytes gone, its length field following"""
    return refig(fig, fig[2:len(fig) - n])


def flag(fig, mask):
    """C/N (0x80), OE (0x40) or P/D (0x20) flipped"""
    return fig[:1] + bytes([fig[1] ^ mask]) + fig[2:]


def pack(fibs_of_figs, n_frames=None):
    """[[FIG, ...] per FIB] -> uint8 [n_frames * 12][32]: each list is one FIB's data field as given (0xFF and zeros behind it)"""
    n = len(fibs_of_figs)
    n_frames = n_frames if n_frames is not None else max(1, -(-n // 12))
    out = np.zeros((n_frames * 12, 32), np.uint8)
    out[:, 0] = 0xFF
    for k, figs in enumerate(fibs_of_figs):
        d = b"".join(figs)
        assert len(d) <= 30, len(d)
        d = (d + (b"\xff" if len(d) < 30 else b"")).ljust(30, b"\x00")
        c = synth.crc16(d)
        out[k] = np.frombuffer(d + bytes([c >> 8, c & 0xFF]), np.uint8)
    return out


def greedy(figs):
    """FIGs into FIBs in order, a new FIB when the next FIG does not fit"""
    fibs, cur = [], []
    for f in figs:
        if sum(map(len, cur)) + len(f) > 30:
            fibs.append(cur)
            cur = []
        cur.append(f)
    if cur:
        fibs.append(cur)
    return fibs


# ------------------------------------------------------------------ an ensemble that gives every call something to list
EEP_UNIT = {0: (12, 8, 6, 4), 1: (27, 21, 18, 15)}


def ensemble(seed, n_audio=3, n_stream=2, n_packet=3, pd=0):
    """-> dict of FIG lists by kind.  Sub-channels: EEP-A, EEP-B and UEP mixed, ids drawn without replacement."""
    rng = np.random.default_rng(seed)
    ids = [int(x) for x in rng.permutation(64)[:n_audio + n_stream + n_packet]]
    start, subs = 0, []
    for k, i in enumerate(ids):
        kind = k % 3
        if kind == 2:
            idx = int(rng.integers(0, 20))
            subs.append({"id": i, "start": start, "uep_index": idx})
            start += dabgpu.uep_subchannel(idx, 0).length
        else:
            level = int(rng.integers(1, 5))
            n = int(rng.integers(1, 4))
            subs.append({"id": i, "start": start, "option": kind, "level": level, "size": EEP_UNIT[kind][level - 1] * n})
            start += subs[-1]["size"]
    assert start <= 864
    sid = lambda k: (0xE0000000 if pd else 0) + 0xC220 + k  # noqa: E731
    services, described, fec, globals_, apps = [], [], [], [], []
    for k in range(n_audio):
        services.append((sid(k), [("audio", 63 if k % 2 else 0, ids[k], 1)]))
        globals_.append((sid(k), 0, "short", ids[k], k % 2))
        apps.append((sid(k), 0, [(2, bytes([0x80 + k])), (7, b"")]))
    for k in range(n_stream):
        i = ids[n_audio + k]
        services.append((sid(10 + k), [("stream", 24 if k % 2 == 0 else 5, i, 1, k % 2), ("fidc", 3, 9 + k)]))
        globals_.append((sid(10 + k), 0, "short", i, 0))
        globals_.append((sid(10 + k), 1, "fidc", 9 + k, 0))
        apps.append((sid(10 + k), 0, [(9, bytes(range(k + 1)))]))
    for k in range(n_packet):
        i = ids[n_audio + n_stream + (k % max(1, n_packet - 1))]   # (the last two components share a sub-channel)
        scid = 0x300 + 17 * k
        services.append((sid(20 + k), [("packet", scid, 1)]))
        described.append({"scid": scid, "subchannel": i, "address": 1 + 100 * k, "dscty": 60 if k % 2 == 0 else 5, "dg_flag": k % 2,
                          "caorg": 0x1234 if k == 1 else None})
        fec.append((i, 1))
        globals_.append((sid(20 + k), 0, "long", scid, k % 2))
        apps.append((sid(20 + k), 0, [(2, b"\x01\x02"), (0x44A, bytes(12))]))
    two = lambda seq: [seq[i:i + 2] for i in range(0, len(seq), 2)]  # noqa: E731
    return {
        "f1": [synth.fig0_1(s) for s in two(subs)],
        "f2": [fig0_2_mixed(s, pd) for s in two(services)],
        "f3": [synth.fig0_3(d) for d in two(described)],
        "f14": [synth.fig0_14(fec)] if fec else [],
        "f8": [fig0_8_any(g, pd) for g in two(globals_)],
        "f13": [synth.fig0_13([a], pd) for a in apps],
        "other": [synth.fig0_0(0xCE15, 1234), synth.fig1(0, 0xCE15, "FIG listings"), synth.fig0_9(0xE1, 2)],
    }


ORDER = ("other", "f1", "f2", "f3", "f14", "f8", "f13")


def figs_of(e, order=ORDER):
    return [f for k in order for f in e[k]]


def build_cases():
    """-> [(name, fib [n_frames * 12][32], crc_ok [n_frames * 12])]"""
    cases = []

    def add(name, fib, crc=None):
        cases.append((name, fib, np.ones(len(fib), np.uint8) if crc is None else np.asarray(crc, np.uint8)))

    for seed in range(4):
        add("plain_%d" % seed, pack(greedy(figs_of(ensemble(seed, pd=seed & 1)))))
    # what pass 1 needs announced in the LAST FIB, behind everything that uses it
    e = ensemble(10)
    add("announced_last", pack(greedy(figs_of(e, ("f13", "f2", "other", "f8", "f14", "f3", "f1")))))
    add("repeated_frames", np.concatenate([pack(greedy(figs_of(e)), 2), pack(greedy(figs_of(ensemble(11))), 2)]))
    add("no_frames", np.zeros((0, 32), np.uint8))
    # every FIG kind cut by one byte and by one field, and its header flags flipped
    fields = {"f1": 3, "f2": 2, "f3": 5, "f14": 1, "f8": 2, "f13": 2}
    for kind, field in fields.items():
        for what, n in (("byte", 1), ("field", field)):
            for which in (0, -1):
                e = ensemble(20 + len(cases))
                e[kind][which] = cut(e[kind][which], n)
                add("cut_%s_%s_%d" % (kind, what, which), pack(greedy(figs_of(e))))
        for what, mask in (("cn", 0x80), ("oe", 0x40), ("pd", 0x20)):
            e = ensemble(60 + len(cases))
            e[kind] = [flag(f, mask) for f in e[kind]]
            add("flag_%s_%s" % (kind, what), pack(greedy(figs_of(e))))
    # FIG 0/1: what dabgpu_fig_subchannels refuses, and what it passes over
    eep = lambda i, start, option, level, size: {"id": i, "start": start, "option": option, "level": level, "size": size}  # noqa: E731
    short = lambda i, start, sw, idx: _bits((i, 6), (start, 10), (0, 1), (sw, 1), (idx, 6))  # noqa: E731
    good = [eep(1, 0, 0, 3, 48), {"id": 2, "start": 48, "uep_index": 7}]
    bad = {
        "reserved_option": [synth.fig0_1(good + [eep(3, 200, 2, 1, 13), eep(4, 300, 7, 4, 0)])],
        "table_switch": [synth.fig0_1(good), fig0(1, short(5, 400, 1, 3))],
        "table_switch_first": [fig0(1, short(5, 400, 1, 3)), synth.fig0_1(good)],
        "size_not_a_multiple_a": [synth.fig0_1(good + [eep(6, 200, 0, 3, 49)])],
        "size_not_a_multiple_b": [synth.fig0_1([eep(6, 200, 1, 2, 22)] + good)],
        "size_zero": [synth.fig0_1(good + [eep(6, 200, 0, 1, 0)])],
        "size_beyond_the_cif": [synth.fig0_1(good + [eep(6, 800, 0, 4, 128)])],
        "uep_beyond_the_cif": [synth.fig0_1(good + [{"id": 7, "start": 860, "uep_index": 63}])],
        "bad_after_duplicate": [synth.fig0_1(good), synth.fig0_1([eep(1, 500, 0, 3, 49), eep(8, 600, 0, 3, 12)])],
        "bad_duplicate_of_bad": [synth.fig0_1([eep(1, 500, 0, 3, 49)]), synth.fig0_1(good)],
        "bad_in_next_config": [synth.fig0_1(good), flag(synth.fig0_1([eep(9, 500, 0, 3, 49)]), 0x80)],
        "bad_in_other_ensemble": [synth.fig0_1(good), flag(synth.fig0_1([eep(9, 500, 0, 3, 49)]), 0x40)],
        "bad_in_other_ensemble_short": [synth.fig0_1(good), flag(fig0(1, short(9, 500, 1, 1)), 0x40)],
        "bad_with_pd": [synth.fig0_1(good), flag(synth.fig0_1([eep(9, 500, 1, 1, 28)]), 0x20)],
        "bad_cut_off": [synth.fig0_1(good), cut(synth.fig0_1([eep(9, 500, 0, 3, 49)]), 1)],
        "bad_behind_cut_short": [cut(synth.fig0_1(good), 1), synth.fig0_1([eep(9, 500, 0, 3, 6), eep(10, 506, 0, 3, 7)])],
    }
    for name, f1 in bad.items():
        e = ensemble(100 + len(cases))
        e["f1"] = f1 + e["f1"]
        add("fig01_" + name, pack(greedy(figs_of(e))))
    e = ensemble(130)
    e["f1"] = [synth.fig0_1([eep(6, 200, 0, 3, 49)])] + e["f1"]
    fib = pack(greedy(figs_of(e, ("f1", "f2", "f3", "f14", "f8", "f13", "other"))))
    crc = np.ones(len(fib), np.uint8)
    crc[0] = 0                                                  # (the refused entry opens FIB 0)
    add("fig01_bad_in_failed_crc", fib, crc)
    # duplicates: SubChId in FIG 0/1 (first start wins), SCId in FIG 0/3, (SId, SCIdS, type) in FIG 0/13, sub-channel in FIG 0/2,
    # (sub-channel, address) in two packet components, FEC scheme twice
    e = ensemble(140)
    first = e["f1"][0]
    e["f1"].append(first[:3] + bytes([first[3] ^ 0x01]) + first[4:])                       # same ids, another start address
    e["f3"].append(synth.fig0_3([{"scid": 0x300, "subchannel": 63, "address": 1000}, {"scid": 0x999, "subchannel": 1, "address": 5}]))
    e["f13"] = e["f13"] + [synth.fig0_13([(0xC220, 0, [(2, b"\xee\xee\xee"), (3, b"")])])]
    e["f2"] = e["f2"] + e["f2"][:1] + [fig0_2_mixed([(0xABCD, [("packet", 0x300, 0), ("packet", 0x999, 1), ("audio", 1, 63, 0)])])]
    e["f14"] += [synth.fig0_14([(i, 3) for i in range(0, 28)]), synth.fig0_14([(i, 2) for i in range(28, 56)])]
    add("duplicates", pack(greedy(figs_of(e))))
    # FIG 0/2: NumComponents larger than the body; a service cut inside its identifier
    for k, (ncomp, tail) in enumerate(((5, 2), (15, 0), (1, 1))):
        e = ensemble(150 + k)
        f = e["f2"][0]
        body = bytearray(f[2:])
        body[2] = (body[2] & 0xF0) | ncomp
        e["f2"][0] = refig(f, bytes(body[:len(body) - tail]))
        add("ncomp_%d_tail_%d" % (ncomp, tail), pack(greedy(figs_of(e))))
    # FIG 0/3 with CAOrg present, whole and cut inside it; FIG 0/8 in its four forms and a FIDC, with 16- and 32-bit SIds
    for k, n in enumerate((0, 1, 2, 3)):
        e = ensemble(160 + k, n_packet=2)
        e["f3"] = [cut(synth.fig0_3([{"scid": 0x300, "subchannel": 40, "address": 77, "caorg": 0xBEEF}]), n)] + e["f3"]
        add("caorg_cut_%d" % n, pack(greedy(figs_of(e))))
    for pd in (0, 1):
        e = ensemble(170 + pd, pd=pd)
        s = (0xE0000000 if pd else 0) + 0xC220
        e["f8"] = [fig0_8_any([(s, 0, "short", 3, 0), (s, 1, "short", 4, 1)], pd), fig0_8_any([(s + 20, 0, "long", 0x300, 0)], pd),
                   fig0_8_any([(s + 21, 0, "long", 0x311, 1), (s, 2, "fidc", 5, 1)], pd), cut(fig0_8_any([(s + 22, 0, "long", 0x322, 1)], pd), 1),
                   cut(fig0_8_any([(s + 22, 3, "short", 9, 0)], pd), 1)] + e["f8"]
        add("fig08_forms_pd%d" % pd, pack(greedy(figs_of(e))))
    # FIG 0/13: an application cut in its header and in its data; data longer than the record keeps
    for k, n in enumerate((1, 2, 3, 18, 20)):
        e = ensemble(180 + k)
        e["f13"] = [cut(synth.fig0_13([(0xC220, 0, [(2, b"\x01\x02"), (0x44A, bytes(range(17)))])]), n)] + e["f13"][1:]
        add("fig013_cut_%d" % n, pack(greedy(figs_of(e))))
    # an end marker and a zero length in the middle of a FIB; a length that runs over the FIB's end; a FIG of another type
    for k, what in enumerate(("marker", "zero_length", "overrun", "type_1", "type_7")):
        e = ensemble(190 + k)
        fibs = greedy(figs_of(e, ("f1", "f2", "f3", "f14", "f8", "f13")))
        fib = pack(fibs)
        at = len(fibs[0][0])                                    # the header of FIB 0's second FIG
        if what == "marker":
            fib[0, at] = 0xFF
        elif what == "zero_length":
            fib[0, at] &= 0xE0
        elif what == "overrun":
            fib[0, at] |= 0x1F
        else:
            fib[0, at] = (fib[0, at] & 0x1F) | ((1 if what == "type_1" else 7) << 5)
        add("fib_" + what, fib)
    # failed CRCs: each FIB of a frame in turn left out, and all of them
    e = ensemble(200)
    fib = pack(greedy(figs_of(e)))
    used = len(greedy(figs_of(e)))
    for k in range(used):
        crc = np.ones(len(fib), np.uint8)
        crc[k] = 0
        add("crc_failed_%d" % k, fib, crc)
    add("crc_failed_all", fib, np.zeros(len(fib), np.uint8))
    # more than a call keeps: all 64 SubChIds as audio and as stream components; more than 256 packet components and applications
    subs = [{"id": i, "start": 13 * i, "option": 0, "level": 4, "size": 4 * (1 + i % 3)} for i in range(64)]
    f1 = [synth.fig0_1(subs[i:i + 7]) for i in range(0, 64, 7)]
    audio = [fig0_2_mixed([(0x1000 + i, [("audio", 63, j, 1) for j in range(i, min(i + 12, 64))])]) for i in range(0, 64, 12)]
    stream = [fig0_2_mixed([(0x2000 + i, [("stream", 24, j, 1, j & 1) for j in range(i, min(i + 12, 64))])]) for i in range(0, 64, 12)]
    add("all_64_subchannels", pack(greedy(f1 + audio + stream)))
    add("all_64_subchannels_one_bad", pack(greedy(f1[:5] + [synth.fig0_1([eep(63, 850, 1, 1, 26)])] + f1[5:] + audio)))
    n_many = 270
    f3 = [synth.fig0_3([{"scid": 0x100 + i, "subchannel": i % 64, "address": 1 + i} for i in range(j, min(j + 5, n_many))]) for j in range(0, n_many, 5)]
    f2 = [fig0_2_mixed([(0x3000 + j, [("packet", 0x100 + i, i & 1) for i in range(j, min(j + 12, n_many))])]) for j in range(0, n_many, 12)]
    add("many_packet_components", pack(greedy(f1 + f3 + f2)))
    f13 = [synth.fig0_13([(0x4000 + j, j % 16, [(i, b"") for i in range(12)])]) for j in range(23)]
    f8 = [fig0_8_any([(0x4000 + j, j % 16, "long", 0x100 + j, 0), (0x4000 + j + 1, (j + 1) % 16, "short", j, 0)]) for j in range(0, 23, 2)]
    add("many_user_applications", pack(greedy(f1 + f3[:6] + f8 + f13)))
    f8 = [fig0_8_any([(0x5000 + i, 0, "long", 0x100 + i, 0) for i in range(j, min(j + 5, n_many))]) for j in range(0, n_many, 5)]
    f13 = [synth.fig0_13([(0x5000 + i, 0, [(4, b"\x00")]) for i in range(j, min(j + 4, n_many))]) for j in range(n_many - 8, n_many, 4)]
    add("many_globals_and_descriptions", pack(greedy(f3 + f8 + f13)))
    return cases


def record():
    cases = build_cases()
    store = {"names": np.array([c[0] for c in cases]), "n_fibs": np.array([len(c[1]) for c in cases], np.int32),
             "fib": np.concatenate([c[1].reshape(-1, 32) for c in cases]), "crc_ok": np.concatenate([c[2] for c in cases])}
    for call in CALLS:
        meta, blobs = [], []
        for _, fib, crc in cases:
            for m, rc, n, out in three_sizes(call, fib, crc):
                meta.append((m, rc, n))
                blobs.append(out)
        store[call + "_meta"] = np.array(meta, np.int32).reshape(len(cases), 3, 3)   # [case][size](max, status, n)
        store[call + "_out"] = np.concatenate(blobs)
        large = store[call + "_meta"][:, 0]
        status = store[call + "_meta"][:, :, 1].ravel()
        nonempty = int(((large[:, 1] == OK) & (large[:, 2] > 0)).sum())
        counts = {s: int((status == s).sum()) for s in sorted(set(status.tolist()))}
        print("%-18s non-empty in %d of %d cases, most %d; statuses %s" % (call, nonempty, len(cases), large[:, 2].max(), counts))
        assert 2 * nonempty >= len(cases), call
        assert counts.get(OK, 0) >= 10 and counts.get(ERR_CAPACITY, 0) >= 10, call
        if call == "subchannels":
            assert counts.get(ERR_PROFILE, 0) >= 10
    np.savez_compressed(PATH, **store)
    size = os.path.getsize(PATH)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != os.path.basename(PATH))
    print("%d cases, %d bytes (largest other fixture: %d)" % (len(cases), size, largest))
    assert size <= largest and size < (1 << 20)


def load():
    """-> (cases [(name, fib, crc_ok)], {call: (meta [case][3][3], out bytes)})"""
    d = np.load(PATH)
    ends = np.cumsum(d["n_fibs"])
    cases = [(str(name), d["fib"][e - k:e], d["crc_ok"][e - k:e]) for name, k, e in zip(d["names"], d["n_fibs"], ends)]
    return cases, {call: (d[call + "_meta"], d[call + "_out"]) for call in CALLS}


if __name__ == "__main__":
    record()
