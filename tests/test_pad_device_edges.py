"""What of dabgpu_pad_labels_dev and dabgpu_mot_slides_dev only device code can get wrong (csrc/pad_kernels.hip,
csrc/mot_kernels.hip, csrc/wave_copy.hpp): the copy classes of the whole-wave copy, the window of an access unit the kernels
fetch into LDS, n_superframes as the device reads it, and every cut of a stream in two launches.  The streams are those of
test_pad_slides.py (its groups "moves", "slotcopies", "window" and "stale" were made for this file); the references are
tests/mot_reference.py and tests/pad_reference.py, byte for byte.  The CPU tests here say what the directed streams reach --
a census of every copy order, from tests/mot_order_census.cpp -- the GPU tests run them."""
import os
import subprocess

import numpy as np
import pytest

import dabgpu

import mot_reference as M
import pad_reference as P
import test_pad_labels as T
import test_pad_slides as S
import wave_copy_mutants as WM
from conftest import ROOT
from test_pad_slides import built_streams, pctx                      # noqa: F401 (fixtures)
from test_wave_copy import CSRC, SANITIZE

DIRECTED = ("moves", "slotcopies")
WINDOW = ("window", "stale")
MOVE, SLIDE = 2, 3
CENSUS_SLOTS, CENSUS_STRIDE = 16, 2048


# ------------------------------------------------------------------------------------------------ the census of copy orders
def build_census(tmp_path, emulate=False, k=0):
    exe = str(tmp_path / ("mot_order_census_%d_%d" % (emulate, k)))
    extra = (["-DEMULATE"] if emulate else []) + (WM.write_mutant(k, tmp_path) if k else [])
    subprocess.check_call(SANITIZE + ["-I" + os.path.join(ROOT, "include")] + extra + [os.path.join(ROOT, "tests", "mot_order_census.cpp"), "-o", exe])
    return exe


def stream_file(tmp_path, name, st):
    path = str(tmp_path / (name + ".stream"))
    stride = 8192 + 128 if st["body_capacity"] > 4096 else CENSUS_STRIDE
    with open(path, "wb") as f:
        f.write(np.array([st["s"], st["body_capacity"], CENSUS_SLOTS, stride, len(st["data"])], np.int32).tobytes())
        f.write(np.ascontiguousarray(st["data"]).tobytes())
        f.write(np.ascontiguousarray(st["status"]).tobytes())
    return path


def run_census(exe, path):
    """-> (exit status, orders [(kind, src, dst, len)], the bytes the orders left, output)"""
    r = subprocess.run([exe, path, path + ".out"], capture_output=True, text=True, timeout=300)
    orders = [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines() if l[:1].isdigit()]
    left = open(path + ".out", "rb").read() if r.returncode == 0 else b""
    return r.returncode, orders, left, r.stdout[-600:] + r.stderr[-1200:]


def classify(src, dst, n):
    """one ORDER_MOVE / ORDER_SLIDE as wave_copy() takes it, arena and slots on 16-byte boundaries (test_pad_slides.call
    asserts that of its buffers, the ABI of its callers) -> (bytes per access, head, words, tail, len < head)"""
    phase = (dst ^ src) & 15
    B = 16 if phase == 0 else 4 if phase & 3 == 0 else 1
    if B == 1:
        return 1, phase & 3, n, 0, False                              # (in the head's place: how far apart the two are, mod 4)
    head = -dst % B
    short, head = n < head, min(head, n)
    words = (n - head) // B
    return B, head, words, n - head - words * B, short


def census(orders):
    """-> {(kind, B): dict(n, heads {head: count}, words {..}, tails {..}, short)}"""
    out = {}
    for kind, src, dst, n in orders:
        if kind not in (MOVE, SLIDE):
            continue
        B, head, words, tail, short = classify(src, dst, n)
        c = out.setdefault((kind, B), dict(n=0, heads={}, words={}, tails={}, short=0))
        c["n"] += 1
        c["short"] += short
        for key, v in (("heads", head), ("words", words), ("tails", tail)):
            c[key][v] = c[key].get(v, 0) + 1
    return out


def table(cs):
    lines = []
    for (kind, B), c in sorted(cs.items()):
        show = lambda d, keys: " ".join("%d:%d" % (k, d.get(k, 0)) for k in keys) + "  other:%d" % sum(v for k, v in d.items() if k not in keys)
        line = "%-5s %2d-byte  copies %3d" % ("MOVE" if kind == MOVE else "SLIDE", B, c["n"])
        if B > 1:
            line += "  heads %s | words %s | tails %s | len < head: %d" % (show(c["heads"], sorted({0, 1, B // 2 - 1, B - 1})), show(c["words"], [0, 1, 63, 64, 65]),
                                                                       show(c["tails"], [0, 1, B - 1]), c["short"])
        else:
            line += "  longer than one trip of the wave (64 bytes): %d | source and destination two bytes apart (mod 4): %d" % (
                sum(v for k, v in c["words"].items() if k > 64), c["heads"].get(2, 0))
        lines.append(line)
    return "\n".join(lines)


def test_census_of_copy_orders(built_streams, tmp_path):
    """Every ORDER_MOVE and ORDER_SLIDE of every stream of test_pad_slides.py, classified as wave_copy() takes it.  The
    directed streams alone ("moves", "slotcopies") must reach, for MOVE and for SLIDE: all three classes (of the byte class
    both kinds: source and destination an odd number of bytes apart, and two); on each word class word counts 0, 1, 63, 64,
    65 (the lane-stride loop not entered, one trip, one trip less a lane, exactly full, a second trip) and tails 0, 1,
    B - 1; for MOVE heads 0, 1, B - 1 and one in between, and a copy with len < head.

    A SLIDE cannot have a head: its source is HEADER_OFF or BODY_OFF of a 16-aligned arena, so wherever source and
    destination share a phase the destination is aligned as well.  The test asserts that, too -- should the arena's layout
    ever change, the census will ask for the heads.

    The directed streams, as printed by this test (all streams together add no MOVE to the two word classes: without the
    directed ones not one segment was ever moved by words):
      MOVE   1-byte  copies  34  longer than one trip of the wave (64 bytes): 9 | source and destination two bytes apart (mod 4): 2
      MOVE   4-byte  copies   8  heads 0:4 1:2 3:1  other:1 | words 0:2 1:2 63:1 64:1 65:1  other:1 | tails 0:2 1:2 3:2  other:2 | len < head: 1
      MOVE  16-byte  copies  10  heads 0:5 1:1 7:1 15:2  other:1 | words 0:3 1:2 63:1 64:1 65:1  other:2 | tails 0:2 1:4 15:2  other:2 | len < head: 1
      SLIDE  1-byte  copies  12  longer than one trip of the wave (64 bytes): 8 | source and destination two bytes apart (mod 4): 1
      SLIDE  4-byte  copies   5  heads 0:5 1:0 3:0  other:0 | words 0:1 1:1 63:1 64:1 65:1  other:0 | tails 0:1 1:2 3:2  other:0 | len < head: 0
      SLIDE 16-byte  copies  25  heads 0:25 1:0 7:0 15:0  other:0 | words 0:1 1:16 63:1 64:1 65:1  other:5 | tails 0:5 1:2 15:2  other:16 | len < head: 0
    (the head in between is 2 of 4, under "other", and 7 of 16; a head clipped by len < head counts as what it is clipped to.)
    """
    exe = build_census(tmp_path)
    per = {}
    for name, st in built_streams.items():
        rc, orders, _left, text = run_census(exe, stream_file(tmp_path, name, st))
        assert rc == 0, (name, text)
        per[name] = orders
    print("all streams:\n" + table(census(sum(per.values(), []))))
    cs = census(sum((per[n] for n in DIRECTED), []))
    print("the directed streams:\n" + table(cs))
    for kind in (MOVE, SLIDE):
        assert {B for k, B in cs if k == kind} == {1, 4, 16}, kind
        assert cs[(kind, 1)]["heads"].get(2) and set(cs[(kind, 1)]["heads"]) & {1, 3}, (kind, cs[(kind, 1)])      # both kinds of byte copy
        for B in (4, 16):
            c = cs[(kind, B)]
            assert set(c["words"]) >= {0, 1, 63, 64, 65} and set(c["tails"]) >= {0, 1, B - 1}, (kind, B, c)
            if kind == MOVE:
                assert set(c["heads"]) >= {0, 1, B - 1} and any(1 < h < B - 1 for h in c["heads"]) and c["short"] >= 1, (B, c)
            else:
                assert set(c["heads"]) == {0} and c["short"] == 0, (B, c)
    assert any(n > 64 for kind, s_, d_, n in sum((per[n] for n in DIRECTED), []) if kind == SLIDE and classify(s_, d_, n)[0] == 1)
    # no stream anywhere gives a SLIDE a head
    assert all(set(c["heads"]) == {0} for (kind, B), c in census(sum(per.values(), [])).items() if kind == SLIDE and B > 1)


@pytest.fixture(scope="module")
def emulated(built_streams, tmp_path_factory):
    """the directed streams through the census with the orders executed by the 64-lane emulation of wave_copy.hpp"""
    tmp = tmp_path_factory.mktemp("emulated")
    exe = build_census(tmp, emulate=True)
    out = {}
    for name in DIRECTED:
        rc, orders, left, text = run_census(exe, stream_file(tmp, name, built_streams[name]))
        assert rc == 0 and left, (name, text)
        out[name] = (orders, left)
    return tmp, out


def test_emulated_wave_leaves_what_the_host_executor_leaves(built_streams, emulated, tmp_path):
    """every stream: arena, slots, state and counters after the orders are the same bytes whether mot::execute() moves them or
    wave_copy() does, lane by lane -- and every byte of every copy has exactly one lane that writes it"""
    plain, wave = build_census(tmp_path), build_census(tmp_path, emulate=True)
    for name, st in built_streams.items():
        path = stream_file(tmp_path, name, st)
        a, b = run_census(plain, path), run_census(wave, path)
        assert a[0] == 0 and b[0] == 0 and a[1] == b[1] and a[2] == b[2] and len(a[2]) > 0, (name, a[3], b[3])


@pytest.mark.parametrize("k", sorted(WM.MUTANTS))
def test_every_mutant_of_the_copy_shows_in_a_directed_stream(built_streams, emulated, k):
    """the census with -DEMULATE -DMUTANT=k on the directed streams: each mutant must leave other bytes in the arena or a
    slot of at least one of them than the header does -- or be stopped on the way, where it leaves the same bytes on this
    machine and is wrong all the same: a byte written by two lanes (status 6: mutant 4), a word access off its alignment
    (UBSan: mutants 6 and 7).  Mutant 1 is the header's equal (wave_copy_mutants.EQUIVALENT): it must leave the same bytes."""
    tmp, want = emulated
    exe = build_census(tmp, emulate=True, k=k)
    seen = []
    for name in DIRECTED:
        rc, orders, left, text = run_census(exe, stream_file(tmp, name, built_streams[name]))
        if rc != 0:
            seen.append((name, "two writers" if rc == 6 else "sanitizer" if "runtime error" in text or "AddressSanitizer" in text else "status %d" % rc))
            assert rc == 6 or "runtime error" in text or "AddressSanitizer" in text, text
        elif left != want[name][1]:
            n = sum(x != y for x, y in zip(left, want[name][1]))
            seen.append((name, "%d bytes differ" % n))
        assert orders == want[name][0][:len(orders)]                  # (the orders are the walk's: no mutant changes them)
    print("mutant %d (%s): %s" % (k, WM.MUTANTS[k][0], seen or "the same bytes"))
    assert (seen == []) if k in WM.EQUIVALENT else seen, "mutant %d (%s) went through the directed streams unseen" % (k, WM.MUTANTS[k][0])


# ------------------------------------------------------------------------------------------------ labels of the new streams
def label_spec(st, a=0, b=None, **kw):
    b = len(st["data"]) if b is None else b
    return dict(dict(s=st["s"], data=st["data"][a:b], status=st["status"][a:b], n=b - a), **kw)


@pytest.mark.parametrize("name", WINDOW)
def test_window_streams_through_the_label_call(built_streams, name):
    """the label beside the slide: host call and reference, scenario by scenario with the state handed on"""
    st = built_streams[name]
    rx, state = P.Receiver(), None
    texts = S.WINDOW_TEXT if name == "window" else S.STALE_TEXT
    for (sc, a, b), text in zip(st["bounds"], texts):
        want = rx.call(st["data"][a:b], st["status"][a:b], b - a, st["s"])
        got = T.call(T.HostMemory(), [label_spec(st, a, b, state=state)])[0]
        assert T.same(got, want), sc.name + T.explain(got, want)
        state = got[2]
        assert T.text_of(want[0]) == text and int(want[1]["labels_completed"][0]) == 1, sc.name
        assert int(want[1]["pad_malformed"][0]) == sc.counts["pad_malformed"] and int(want[1]["groups_ok"][0]) == 2, (sc.name, want[1])


# ------------------------------------------------------------------------------------------------------------ GPU
def misplaced(st, **kw):
    """the stream at every base offset 1 .. 15 off a 256-byte boundary, row strides of 110 s + 0, 1, 3"""
    return [dict(kw, data_off=off, stride=110 * st["s"] + [0, 1, 3][off % 3]) for off in range(1, 16)]


@pytest.mark.gpu
def test_gpu_fetch_window_slides(pctx, built_streams):
    """the window and stale-row streams, each at 15 base offsets and three row strides, in one call: slides, counters, state
    and arena equal the reference and the host call"""
    specs, wants = [], []
    for name in WINDOW:
        st = built_streams[name]
        base = S.spec_of(st, 0, len(st["data"]), max_slides=8, slide_stride=1024)
        want = S.ref_call(M.Receiver(st["body_capacity"]), base)
        assert len(want[0]) == len(st["bounds"])
        for extra in misplaced(st):
            specs.append(dict(base, **extra))
            wants.append((name, want))
    got, host = S.call(S.DeviceMemory(pctx), specs), S.call(S.HostMemory(), specs)
    for sp, g, h, (name, w) in zip(specs, got, host, wants):
        assert S.same(g, w), (name, sp["data_off"]) + (S.explain(g, w),)
        assert S.same(h, w) and g["state"].tobytes() == h["state"].tobytes() and (g["arena"] == h["arena"]).all(), (name, sp["data_off"])


@pytest.mark.gpu
def test_gpu_fetch_window_labels(pctx, built_streams):
    """the same through the label call: label, counters and state"""
    specs, wants = [], []
    for name in WINDOW:
        st = built_streams[name]
        want = P.Receiver().call(st["data"], st["status"], len(st["data"]), st["s"])
        assert T.text_of(want[0]) == (S.WINDOW_TEXT if name == "window" else S.STALE_TEXT)[-1]
        for extra in misplaced(st):
            specs.append(label_spec(st, **extra))
            wants.append((name, want))
    got, host = T.call(T.DeviceMemory(pctx), specs), T.call(T.HostMemory(), specs)
    for sp, g, h, (name, w) in zip(specs, got, host, wants):
        assert T.same(g, w), (name, sp["data_off"]) + (T.explain(g, w),)
        assert T.same(h, w) and g[2].tobytes() == h[2].tobytes(), (name, sp["data_off"])


N_SUPERFRAMES = [-1, 0, 4, 5, 2 ** 31 - 1]
MAX_SF = 4


def ff_behind(st, a, b):
    """rows a .. b of the stream, and two rows of 0xFF behind them"""
    ff = np.full((2, 110 * st["s"]), 0xFF, np.uint8)
    ffs = np.full(2 * 64, 0xFF, np.uint8).view(P.STATUS_DTYPE)
    return np.concatenate([st["data"][a:b], ff]), np.concatenate([st["status"][a:b], ffs])


@pytest.mark.gpu
def test_gpu_n_superframes_as_the_slide_call_reads_it(pctx, built_streams):
    """follow records that say -1, 0, max_superframes, one more and INT32_MAX, in front of max_superframes = 4 rows with rows
    of 0xFF behind them, the state and the arena of two super-frames before handed in: what the reference gives for
    clamp(n, 0, max) rows, nothing of the rows behind; for no rows the state record as it came and counters of zero.  And a
    foreign state record with no rows: a fresh one."""
    st = built_streams["chunks"]
    before = S.call(S.HostMemory(), [S.spec_of(st, 0, 2, max_slides=8, slide_stride=2048)])[0]
    data, status = ff_behind(st, 2, 2 + MAX_SF)
    base = dict(s=st["s"], data=data, status=status, max_sf=MAX_SF, body_capacity=st["body_capacity"], max_slides=8, slide_stride=2048)
    specs = [dict(base, n=n, state=before["state"], arena=before["arena"]) for n in N_SUPERFRAMES]
    noise = np.random.default_rng(3).integers(0, 256, dabgpu.mot_state_bytes(), dtype=np.uint8)
    specs.append(dict(base, n=0, state=noise))
    got, host = S.call(S.DeviceMemory(pctx), specs), S.call(S.HostMemory(), specs)
    for sp, g, h in zip(specs[:-1], got, host):
        rows = min(max(sp["n"], 0), MAX_SF)
        rx = M.Receiver(st["body_capacity"])
        rx.call(st["data"], st["status"], 2, st["s"], 8, 2048)
        want = rx.call(st["data"][2:], st["status"][2:], rows, st["s"], 8, 2048)
        assert S.same(g, want), (sp["n"],) + (S.explain(g, want),)
        assert S.same(h, want) and g["state"].tobytes() == h["state"].tobytes() and (g["arena"] == h["arena"]).all(), sp["n"]
        if rows == 0:
            assert g["state"].tobytes() == before["state"].tobytes() and (g["arena"] == before["arena"]).all() and not g["result"].tobytes().strip(b"\0")
        else:
            assert int(g["result"]["aus"][0]) == 3 * MAX_SF and int(g["result"]["aus_lost"][0]) == 0
    fresh = np.zeros(dabgpu.mot_state_bytes(), np.uint8)
    fresh[S_BODY_CAPACITY_AT:S_BODY_CAPACITY_AT + 4] = np.array([st["body_capacity"]], np.int32).view(np.uint8)
    assert got[-1]["state"].tobytes() == fresh.tobytes() == host[-1]["state"].tobytes() and not got[-1]["result"].tobytes().strip(b"\0")


S_BODY_CAPACITY_AT = 20                                               # dabgpu_mot::State::body_capacity


@pytest.mark.gpu
def test_gpu_n_superframes_as_the_label_call_reads_it(pctx, built_streams):
    """the same for the label call: label, counters and state"""
    st = built_streams["chunks"]
    before = T.call(T.HostMemory(), [label_spec(st, 0, 2)])[0]
    data, status = ff_behind(st, 2, 2 + MAX_SF)
    specs = [dict(s=st["s"], data=data, status=status, max_sf=MAX_SF, n=n, state=before[2]) for n in N_SUPERFRAMES]
    specs.append(dict(specs[1], state=np.random.default_rng(4).integers(0, 256, dabgpu.pad_state_bytes(), dtype=np.uint8)))
    got, host = T.call(T.DeviceMemory(pctx), specs), T.call(T.HostMemory(), specs)
    for sp, g, h in zip(specs[:-1], got, host):
        rows = min(max(sp["n"], 0), MAX_SF)
        rx = P.Receiver()
        rx.call(st["data"], st["status"], 2, st["s"])
        want = rx.call(st["data"][2:], st["status"][2:], rows, st["s"])
        assert T.same(g, want), (sp["n"],) + (T.explain(g, want),)
        assert T.same(h, want) and g[2].tobytes() == h[2].tobytes(), sp["n"]
        if rows == 0:
            assert g[2].tobytes() == before[2].tobytes() and g[0].tobytes() == before[0].tobytes() and not g[1].tobytes().strip(b"\0")
        else:
            assert int(g[1]["aus"][0]) == 3 * MAX_SF
    assert not got[-1][2].tobytes().strip(b"\0") and not got[-1][1].tobytes().strip(b"\0") and got[-1][2].tobytes() == host[-1][2].tobytes()


CUT_STREAMS = ("chunks",) + DIRECTED + WINDOW
CUT_SLOTS, CUT_STRIDE = 12, 2048


def two_launches(pctx, built_streams, make_entry, outputs):
    """call 1: one entry per (stream, cut c) over rows [0, c); call 2: the matching entries over [c, end) with call 1's state
    (and whatever `outputs` keeps in place); nothing waits between the calls.  make_entry(st, bufs, k, data, status, follow,
    rows left, state in, state out) -> entry; outputs(st) -> dict of per-(stream, cut) device tensors.  -> [(name, c, bufs)]"""
    import torch
    runs, calls = [], ([], [])
    for name in CUT_STREAMS:
        st = built_streams[name]
        n = len(st["data"])
        data = torch.from_numpy(np.ascontiguousarray(st["data"])).cuda()
        status = torch.from_numpy(st["status"].view(np.uint8).reshape(n, 64).copy()).cuda()
        for c in range(n + 1):
            fr = np.zeros(2, dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)
            fr["n_superframes"], fr["synced"] = [c, n - c], 1
            bufs = dict(outputs(st), data=data, status=status, follow=torch.from_numpy(fr.view(np.uint8).reshape(2, 32).copy()).cuda())
            for k, first in enumerate((0, c)):
                row = min(first, n - 1)                               # (a call of no super-frames keeps a row)
                calls[k].append(make_entry(st, bufs, k, data[row].data_ptr(), status[row].data_ptr(), bufs["follow"][k].data_ptr(), n - row,
                                           bufs["states"][0].data_ptr() if k else None, bufs["states"][k].data_ptr()))
            runs.append((name, c, bufs))
    return runs, calls


@pytest.mark.gpu
def test_gpu_every_cut_in_two_launches_slides(pctx, built_streams):
    """the chunking stream and the directed ones cut at EVERY super-frame boundary, all cuts of all streams side by side in
    two launches, state records and arenas staying on the device: slides and summed counters equal the uncut reference, the
    last state record the uncut host run's"""
    import torch
    nb = dabgpu.mot_state_bytes()

    def outputs(st):
        return dict(states=torch.zeros((2, nb), dtype=torch.uint8, device="cuda"),
                    arena=torch.full((dabgpu.mot_arena_bytes(st["body_capacity"]),), S.FILL, dtype=torch.uint8, device="cuda"),
                    slides=torch.full((2, CUT_SLOTS, CUT_STRIDE), S.FILL, dtype=torch.uint8, device="cuda"),
                    results=torch.zeros((2, 128), dtype=torch.uint8, device="cuda"))

    def entry(st, b, k, data, status, follow, rows, state_in, state_out):
        return dabgpu.MotEntry(data, 110 * st["s"], status, follow, 8 * st["s"], rows, state_in, state_out, b["arena"].data_ptr(), b["arena"].numel(),
                               b["slides"][k].data_ptr(), CUT_STRIDE, CUT_SLOTS, 0, b["results"][k].data_ptr())

    runs, calls = two_launches(pctx, built_streams, entry, outputs)
    pctx.mot_slides_dev(calls[0])
    pctx.mot_slides_dev(calls[1])                                    # nothing waits between the calls
    pctx.sync()
    whole = {}
    for name, c, b in runs:
        st = built_streams[name]
        if name not in whole:
            ref = M.Receiver(st["body_capacity"]).call(st["data"], st["status"], len(st["data"]), st["s"], CUT_SLOTS, CUT_STRIDE)
            host = S.run_cut(S.HostMemory, st, [], max_slides=CUT_SLOTS)
            assert S.strip(host[0]) == S.strip(ref[0]) and host[1] == M.total([ref[1]])
            whole[name] = (S.strip(ref[0]), M.total([ref[1]]), host[2].tobytes())
        res = b["results"].cpu().numpy().view(dabgpu.MOT_RESULT_DTYPE).reshape(2)
        raw = b["slides"].cpu().numpy()
        slides = []
        for k in range(2):
            written = int(res[k]["slides_written"])
            for j in range(written):
                rec = raw[k, j, :32].copy().view(dabgpu.MOT_SLIDE_DTYPE)
                hb, bb = int(rec["header_bytes"][0]), int(rec["body_bytes"][0])
                slides.append((rec, raw[k, j, 32:32 + hb].tobytes(), raw[k, j, 32 + hb:32 + hb + bb].tobytes()))
                assert (raw[k, j, 32 + hb + bb:] == S.FILL).all(), (name, c)
            assert (raw[k, written:] == S.FILL).all(), (name, c)
        assert S.strip(slides) == whole[name][0], (name, c)
        assert M.total([res[k:k + 1] for k in range(2)]) == whole[name][1], (name, c)
        assert b["states"][1].cpu().numpy().tobytes() == whole[name][2], (name, c)
    assert len(runs) >= 40 and {name for name, _c, _b in runs} == set(CUT_STREAMS)


@pytest.mark.gpu
def test_gpu_every_cut_in_two_launches_labels(pctx, built_streams):
    """the same through the label call: the label after the second launch, the summed counters and the last state record
    equal the uncut reference and host run"""
    import torch
    nb = dabgpu.pad_state_bytes()

    def outputs(st):
        return dict(states=torch.zeros((2, nb), dtype=torch.uint8, device="cuda"), labels=torch.zeros((2, 144), dtype=torch.uint8, device="cuda"),
                    results=torch.zeros((2, 64), dtype=torch.uint8, device="cuda"))

    def entry(st, b, k, data, status, follow, rows, state_in, state_out):
        return dabgpu.PadEntry(data, 110 * st["s"], status, follow, 8 * st["s"], rows, state_in, state_out, b["labels"][k].data_ptr(), b["results"][k].data_ptr())

    runs, calls = two_launches(pctx, built_streams, entry, outputs)
    pctx.pad_labels_dev(calls[0])
    pctx.pad_labels_dev(calls[1])                                    # nothing waits between the calls
    pctx.sync()
    whole, labelled = {}, 0
    for name, c, b in runs:
        st = built_streams[name]
        if name not in whole:
            ref = P.Receiver().call(st["data"], st["status"], len(st["data"]), st["s"])
            host = T.call(T.HostMemory(), [label_spec(st)])[0]
            assert T.same(host, ref)
            whole[name] = (ref[0].tobytes(), P.total([ref[1]]), host[2].tobytes())
            labelled += int(ref[0]["length"][0]) > 0
        res = b["results"].cpu().numpy().view(dabgpu.PAD_RESULT_DTYPE).reshape(2)
        assert b["labels"][1].cpu().numpy().tobytes() == whole[name][0], (name, c)
        assert P.total([res[k:k + 1] for k in range(2)]) == whole[name][1], (name, c)
        assert b["states"][1].cpu().numpy().tobytes() == whole[name][2], (name, c)
    assert labelled >= 3
