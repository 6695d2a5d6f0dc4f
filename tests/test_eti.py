"""ETI(NI) output (include/dabgpu.h, "ETI(NI) output"): the host-side layout and reader and the device call that writes
a decode call's buffers as 6144-byte frames, held byte for byte to tests/eti_reference.py -- a writer and reader made
from the definition alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dabgpu
import eti_reference as R
from conftest import ROOT, make_ctx
from dabgpu import synth

CSRC = os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd", "csrc")


# ------------------------------------------------------------------ configurations
def ref_stream(scid, sc):
    return {"id": scid, "start": sc.start_address, "bitrate": sc.bitrate_kbps, "uep": bool(sc.is_uep),
            "eep_type": sc.eep_type, "level": sc.protection_level}


def multiplex18():
    """The 18-sub-channel multiplex of the decoder's timing (tools/vit_time.py): 10 x 64 + 4 x 48 (EEP 3-A), 3 x 32
    (EEP 2-A) and one UEP service, 856 CUs; listed here in a scrambled order with ids that do not follow it."""
    scs, cu = [], 0
    for br, lvl, k in ((64, 3, 10), (48, 3, 4), (32, 2, 3)):
        for _ in range(k):
            x = dabgpu.subchannel(cu, br, level=lvl)
            scs.append(x)
            cu += x.length
    scs.append(dabgpu.uep_subchannel(35, cu))
    order = [(7 * i + 3) % 18 for i in range(18)]
    return [((5 * i + 11) % 64, scs[i]) for i in order]


CONFIGS = {
    "one_eep_a": lambda: [(5, dabgpu.subchannel(0, 64, level=3))],
    "multiplex18": multiplex18,
    "uep_and_eep_b": lambda: [(9, dabgpu.subchannel(200, 32, level=2, eep_type=1)), (63, dabgpu.uep_subchannel(17, 100)),
                              (0, dabgpu.subchannel(0, 48, level=1))],
    "full_cif": lambda: [(33, dabgpu.subchannel(0, 1728, level=4))],          # 216 x 4 CUs = 864
    "tiny": lambda: [(1, dabgpu.subchannel(10, 8, level=4))],
    "fic_only": lambda: [],
}


def reference_header(streams, count=0):
    """Bytes before the FIC of the reference writer's frame for these streams."""
    ref = [ref_stream(i, sc) for i, sc in streams]
    frame = R.write_frame(ref, count, bytes(96), {st["id"]: bytes(st["bitrate"] * 3) for st in ref}, 0xFF)
    return frame[:12 + 4 * len(ref)]


# ------------------------------------------------------------------ CPU
def test_struct_layouts_match_the_header(tmp_path):
    structs = [("dabgpu_eti_stream", dabgpu.EtiStream), ("dabgpu_eti_plan", dabgpu.EtiPlan), ("dabgpu_eti_info", dabgpu.EtiInfo)]
    records = [("dabgpu_eti_status", dabgpu.ETI_STATUS_DTYPE), ("dabgpu_eti_history", dabgpu.ETI_HISTORY_DTYPE)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dabgpu.h"', 'int main(void) {']
    for cname, fields in [(c, [f for f, _ in cls._fields_]) for c, cls in structs] + [(c, list(dt.names)) for c, dt in records]:
        lines.append('  printf("%s %%zu", sizeof(%s));' % (cname, cname))
        lines += ['  printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f in fields]
        lines.append('  printf("\\n");')
    lines.append('  printf("%d %d %d\\n", DABGPU_ETI_FRAME_BYTES, DABGPU_ETI_MAX_STREAMS, DABGPU_ETI_FIC_DELAY);')
    lines.append('  printf("%d %d %d %d\\n", DABGPU_ETI_WARMUP, DABGPU_ETI_FIB_CRC, DABGPU_ETI_NO_ANCHOR, DABGPU_ETI_COUNT_MISMATCH);')
    lines += ['  return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    for (cname, cls), line in zip(structs, out):
        want = [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
        assert line.split()[0] == cname and [int(x) for x in line.split()[1:]] == want, (cname, line, want)
    for (cname, dt), line in zip(records, out[len(structs):]):
        want = [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
        assert line.split()[0] == cname and [int(x) for x in line.split()[1:]] == want, (cname, line, want)
    assert out[5].split() == ["6144", "64", "15"]
    assert [int(x) for x in out[6].split()] == [dabgpu.ETI_WARMUP, dabgpu.ETI_FIB_CRC, dabgpu.ETI_NO_ANCHOR, dabgpu.ETI_COUNT_MISMATCH] \
        == [R.WARMUP, R.FIB_CRC, R.NO_ANCHOR, R.COUNT_MISMATCH]
    assert dabgpu.eti_history_bytes() == dabgpu.ETI_HISTORY_DTYPE.itemsize == 1504


@pytest.mark.parametrize("name", ["one_eep_a", "multiplex18", "uep_and_eep_b", "full_cif", "tiny", "fic_only"])
def test_layout_against_the_reference_header(built, name):
    streams = CONFIGS[name]()
    plan = dabgpu.eti_layout(streams)
    want = reference_header(streams)                       # count 0: ERR 0xFF, even FSYNC, FCT = FP = 0
    n = len(streams)
    got = bytes(plan.header[:12 + 4 * n])
    # the plan's header leaves ERR, FSYNC, FCT, FP and the CRC zero
    assert got[:4] == bytes(4) and got[-2:] == bytes(2)
    assert got[4:-2] == want[4:-2]
    fl, length = R.frame_length([ref_stream(i, sc) for i, sc in streams])
    assert (plan.nst, plan.fl, plan.length, plan.header_bytes) == (n, fl, length, 12 + 4 * n)
    assert plan.data_bytes == sum(sc.bitrate_kbps * 3 for _, sc in streams)
    order = list(plan.order[:n])
    assert sorted(order) == list(range(n))
    assert [streams[k][1].start_address for k in order] == sorted(sc.start_address for _, sc in streams)
    off = 0
    for k in range(n):
        assert (plan.offset[k], plan.bytes[k]) == (off, streams[order[k]][1].bitrate_kbps * 3)
        off += plan.bytes[k]
    if name == "full_cif":
        assert streams[0][1].length == 864 and length == 16 + 96 + 5184 + 8


def test_layout_refusals(built):
    ok = dabgpu.subchannel(0, 64, level=3)                                   # 48 CUs

    def refused(streams):
        with pytest.raises(dabgpu.DabGpuError) as e:
            dabgpu.eti_layout(streams)
        return e.value.status == -1
    assert dabgpu.eti_layout([(1, ok), (2, dabgpu.subchannel(48, 64, level=3))]).nst == 2
    assert refused([(1, ok), (2, dabgpu.subchannel(47, 64, level=3))])      # overlap by one capacity unit
    assert refused([(64, ok)]) and refused([(-1, ok)])                        # id
    assert dabgpu.eti_layout([(i, dabgpu.subchannel(4 * i, 8, level=4)) for i in range(64)]).nst == 64
    arr = (dabgpu.EtiStream * 65)(*[dabgpu.EtiStream(i % 64, dabgpu.subchannel(4 * i, 8, level=4)) for i in range(65)])
    assert dabgpu.lib().dabgpu_eti_layout(arr, 65, C.byref(dabgpu.EtiPlan())) == -1   # 65 streams
    assert refused([(1, dabgpu.Subchannel(0, 9, 0, 0, 3, 12))])              # bit rate 12
    assert refused([(1, dabgpu.Subchannel(0, 9, 0, 0, 3, 0))])
    # frame too long: three streams of 2000 kbit/s are 18 000 bytes per CIF (the sizes in CUs do not overlap)
    assert refused([(i, dabgpu.Subchannel(100 * i, 100, 0, 0, 3, 2000)) for i in range(3)])
    assert refused([(1, dabgpu.Subchannel(860, 5, 0, 0, 3, 8))])             # beyond CU 863
    assert refused([(1, dabgpu.Subchannel(0, 6, 0, 0, 5, 8))]) and refused([(1, dabgpu.Subchannel(0, 6, 0, 2, 3, 8))])
    assert dabgpu.lib().dabgpu_eti_layout(None, 1, C.byref(dabgpu.EtiPlan())) == -1


def _reference_frame(streams, count, seed, crc_ok=(1, 1, 1)):
    rng = np.random.default_rng(seed)
    ref = [ref_stream(i, sc) for i, sc in streams]
    fic = synth.pack_fibs([synth.fig0_0(0xC181, count)] * 3 + [bytes([0x3D]) + bytes(29)] * 2)[:3]
    data = {st["id"]: rng.integers(0, 256, st["bitrate"] * 3, dtype=np.uint8).tobytes() for st in ref}
    return R.write_frame(ref, count, fic.tobytes(), data, R.err_byte(crc_ok)), fic, data


@pytest.mark.parametrize("name", ["one_eep_a", "multiplex18", "uep_and_eep_b", "full_cif", "fic_only"])
def test_parse_accepts_reference_frames(built, name):
    streams = CONFIGS[name]()
    for count in (0, 249, 251, 4999, 1234):
        frame, fic, data = _reference_frame(streams, count, count)
        got = dabgpu.eti_parse(frame)
        want = R.read_frame(frame)
        assert (got["err"], got["fct"], got["fp"], got["nst"], got["fl"], got["length"]) == \
            (want["err"], want["fct"], want["fp"], want["nst"], want["fl"], want["length"])
        assert got["fct"] == count % 250 and got["fp"] == count % 8
        assert got["fic"].tobytes() == want["fic"] == fic.tobytes()
        for g, w in zip(got["streams"], want["streams"]):
            assert (g["scid"], g["sad"], g["tpl"], g["stl"]) == (w["scid"], w["sad"], w["tpl"], w["stl"])
            assert g["data"].tobytes() == w["data"] == data[g["scid"]]
        assert [s["sad"] for s in got["streams"]] == sorted(sc.start_address for _, sc in streams)


def test_parse_rejects_every_single_corruption(built):
    streams = CONFIGS["uep_and_eep_b"]()
    frame, _, _ = _reference_frame(streams, 777, 1)
    info = R.read_frame(frame)
    nst = info["nst"]
    hdr_crc, fic0, data0 = 10 + 4 * nst, 12 + 4 * nst, 12 + 4 * nst + 96
    eof = info["length"] - 8

    def flipped(pos, bit=0):
        b = bytearray(frame)
        b[pos] ^= 1 << bit
        return bytes(b)
    cases = {"FCT": flipped(4, 1), "NST": flipped(5, 0), "FL": flipped(7, 2), "STC sad": flipped(9, 3), "STC stl": flipped(11, 0),
             "MNSC": flipped(8 + 4 * nst, 7), "header CRC": flipped(hdr_crc, 5), "header CRC low": flipped(hdr_crc + 1),
             "FIC": flipped(fic0 + 40, 6), "payload first": flipped(data0), "payload last": flipped(eof - 1, 7),
             "data CRC": flipped(eof, 2), "data CRC low": flipped(eof + 1, 4), "FICF": flipped(5, 7), "MID": flipped(6, 4)}
    # FSYNC of the other parity, FCT left alone
    b = bytearray(frame)
    b[1:4] = R.FSYNC_EVEN if info["fct"] & 1 else R.FSYNC_ODD
    cases["FSYNC parity"] = bytes(b)
    cases["FSYNC bit"] = flipped(2, 3)
    # FL that does not follow from the STC, under a header CRC made right for it
    b = bytearray(frame)
    b[7] ^= 2
    c = synth.crc16(bytes(b[4:hdr_crc]))
    b[hdr_crc:hdr_crc + 2] = bytes([c >> 8, c & 0xFF])
    cases["FL inconsistent with STC"] = bytes(b)
    dabgpu.eti_parse(frame)
    for what, bad in cases.items():
        with pytest.raises(ValueError):
            R.read_frame(bad)
        with pytest.raises(ValueError):
            dabgpu.eti_parse(bad)
            pytest.fail(what + " accepted")
    # what no CRC covers is not judged
    dabgpu.eti_parse(flipped(0, 1))
    dabgpu.eti_parse(flipped(6143))


def test_known_answer_frame():
    """One tiny frame written out (computed once by the reference writer and pasted): a single 8 kbit/s EEP 4-A
    sub-channel (id 1, start 10), CIF count 1251, payload 00..17, FIC = 96 bytes 0xA5, one FIB failed.  Pins the
    reference writer itself; the header fields can be checked by hand."""
    st = [{"id": 1, "start": 10, "bitrate": 8, "uep": False, "eep_type": 0, "level": 4}]
    frame = R.write_frame(st, 1251, b"\xa5" * 96, {1: bytes(range(24))}, 0xE1)
    want = ("e1"                   # ERR
            "f8c549"               # FSYNC: FCT is odd
            "01"                   # FCT = 1251 % 250
            "81"                   # FICF = 1, NST = 1
            "6820"                 # FP = 1251 % 8 = 3 (011), MID = 1 (01), FL = 1 + 1 + 24 + 2 * 3 = 32 (000 0010 0000)
            "040a8c03"             # SCID 1 (000001), SAD 10 (00 0000 1010), TPL 0x23 = EEP, A, level 4 (100011), STL 3
            "ffff"                 # MNSC
            "4edc"                 # CRC of the ten bytes from FCT
            + "a5" * 96            # FIC
            + bytes(range(24)).hex()
            + "561d"               # CRC of FIC + payload
            "ffff"                 # RFU
            "ffffffff"             # TIST
            + "55" * 6000)
    assert frame.hex() == want and len(frame) == 6144
    assert R.read_frame(frame)["length"] == 144 == 4 * 32 + 16


def _kernel_metadata(notes):
    from test_device_asm import kernel_metadata
    return kernel_metadata(notes)


def test_eti_kernels_use_no_scratch_and_spill_nothing(built):
    obj = os.path.join(CSRC, "eti_kernels.o")
    tools = "/opt/rocm/lib/llvm/bin/"
    if not os.path.exists(obj):
        subprocess.check_call(["make", "-C", CSRC, "eti_kernels.o"], stdout=subprocess.DEVNULL)
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "eti.fat"), os.path.join(td, "eti.co")
        subprocess.check_call([tools + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([tools + "clang-offload-bundler", "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + fat, "--output=" + co])
        md = _kernel_metadata(subprocess.check_output([tools + "llvm-readelf", "--notes", co], text=True))
        asm = subprocess.check_output([tools + "llvm-objdump", "-d", co], text=True)
    names = sorted(md, key=lambda k: "eti_frame_kernel" in k)
    assert len(names) == 2 and "eti_anchor_kernel" in names[0] and "eti_frame_kernel" in names[1], names
    for k, v in md.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v.get("agpr_count", 0) == 0 and v["vgpr_count"] <= 64, (k, v)           # 8 waves per SIMD
    # four frames in LDS per workgroup: at least 5 workgroups per CU
    assert md[names[1]]["group_segment_fixed_size"] <= 160 * 1024 // 5
    # results leave through vector stores only
    assert not re.search(r"\bs_(buffer_|scratch_)?(store|atomic)", asm) and re.search(r"global_store_dwordx4", asm)


# ------------------------------------------------------------------ GPU
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_shifted(torch, a, shift):
    """`a` on the device, `shift` bytes behind a 256-byte boundary"""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    room = torch.full((a.size + 256,), 0xEE, dtype=torch.uint8, device="cuda")
    assert room.data_ptr() % 256 == 0
    view = room[shift:shift + a.size]
    view.copy_(torch.from_numpy(a))
    return view


def run_eti(ctx, streams, fib, ok, outs, history=None, cif_start=None, want_history=True, out_shift=0):
    """eti_frames_dev on host arrays: fib [n_streams][n_cif][3][32], ok [n_streams][n_cif][3], outs[i] [n_streams][n_cif]
    [bytes] in the order of `streams` -> eti [n_streams][n_cif][6144], status, history (numpy).  out_shift: the bytes every
    d_out pointer lies behind a 256-byte boundary (8: aligned as the contract asks and no further)."""
    import torch
    n_streams, n_cif = fib.shape[:2]
    plan = dabgpu.eti_layout(streams)
    d_fib, d_ok = _dev(torch, fib), _dev(torch, ok)
    d_outs = [_dev_shifted(torch, o, out_shift) if out_shift else _dev(torch, o) for o in outs]
    assert all(o.data_ptr() % 256 == out_shift for o in d_outs if o.numel())
    d_eti = torch.zeros((n_streams, n_cif, 6144), dtype=torch.uint8, device="cuda")
    d_status = torch.zeros((n_streams, n_cif, 8), dtype=torch.uint8, device="cuda")
    d_hin = None if history is None else _dev(torch, history.view(np.uint8).reshape(n_streams, -1))
    d_hout = torch.zeros((n_streams, 1504), dtype=torch.uint8, device="cuda") if want_history else None
    d_start = None if cif_start is None else _dev(torch, np.asarray(cif_start, np.int32))
    ctx.eti_frames_dev(plan, n_streams, n_cif // 4, d_fib.data_ptr(), d_ok.data_ptr(), [o.data_ptr() for o in d_outs],
                       d_eti.data_ptr(), d_status.data_ptr(), d_history_in=None if d_hin is None else d_hin.data_ptr(),
                       d_history_out=None if d_hout is None else d_hout.data_ptr(),
                       d_cif_start=None if d_start is None else d_start.data_ptr())
    ctx.sync()
    hist = None if d_hout is None else d_hout.cpu().numpy().view(dabgpu.ETI_HISTORY_DTYPE).reshape(n_streams)
    return d_eti.cpu().numpy(), d_status.cpu().numpy().view(dabgpu.ETI_STATUS_DTYPE).reshape(n_streams, n_cif), hist


def make_case(rng, streams, n_streams, n_cif, start_counts, eid=0xC181):
    """Random decoder outputs with FIG 0/0 first in every CIF's first FIB: fib, ok (all 1), outs."""
    fib = np.zeros((n_streams, n_cif, 3, 32), np.uint8)
    for s in range(n_streams):
        for c in range(n_cif):
            figs = [synth.fig0_0(eid, (start_counts[s] + c) % 5000), bytes([0x3D]) + rng.integers(0, 256, 29, dtype=np.uint8).tobytes()]
            figs += [bytes([0x3D]) + rng.integers(0, 256, 29, dtype=np.uint8).tobytes()] * 2
            fib[s, c] = synth.pack_fibs(figs)[:3]
    ok = np.ones((n_streams, n_cif, 3), np.uint8)
    outs = [rng.integers(0, 256, (n_streams, n_cif, sc.bitrate_kbps * 3), dtype=np.uint8) for _, sc in streams]
    return fib, ok, outs


def check_against_reference(streams, fib, ok, outs, eti, status, history=None, cif_start=None, hist_out=None):
    """Every stream's frames and status records equal the reference writer's; -> the reference's histories."""
    ref = [ref_stream(i, sc) for i, sc in streams]
    hists = []
    for s in range(fib.shape[0]):
        data = {st["id"]: outs[k][s] for k, st in enumerate(ref)}
        frames, stat, h = R.write_stream(ref, fib[s], ok[s], data, None if history is None else history[s],
                                         None if cif_start is None else int(cif_start[s]))
        hists.append(h)
        for t, f in enumerate(frames):
            got = eti[s, t].tobytes()
            if got != f:
                diff = [i for i in range(6144) if got[i] != f[i]]
                pytest.fail("stream %d frame %d differs at bytes %s..." % (s, t, diff[:8]))
            assert (int(status[s, t]["cif_count"]), int(status[s, t]["flags"]), int(status[s, t]["fib_ok"]),
                    int(status[s, t]["length"]), int(status[s, t]["reserved"])) == stat[t] + (0,), (s, t, status[s, t], stat[t])
            assert dabgpu.eti_parse(eti[s, t])["fct"] == stat[t][0] % 250
        if hist_out is not None:
            n = len(h["fibs"])
            assert int(hist_out[s]["valid"]) == n and int(hist_out[s]["next_count"]) == h["next_count"]
            assert hist_out[s]["fib"][15 - n:].tobytes() == b"".join(np.asarray(x, np.uint8).tobytes() for x in h["fibs"])
            assert hist_out[s]["crc_ok"][15 - n:].tobytes() == b"".join(np.asarray(x, np.uint8).tobytes() for x in h["crc_ok"])
    return hists


@pytest.fixture(scope="module")
def ectx(built):
    c = make_ctx(None, max_frames=64)
    yield c
    c.close()


def ref_history_to_record(hists):
    rec = np.zeros(len(hists), dabgpu.ETI_HISTORY_DTYPE)
    for s, h in enumerate(hists):
        n = len(h["fibs"])
        rec[s]["valid"], rec[s]["next_count"] = n, h["next_count"]
        if n:
            rec[s]["fib"][15 - n:] = np.asarray(h["fibs"], np.uint8).reshape(n, 96)
            rec[s]["crc_ok"][15 - n:] = np.asarray(h["crc_ok"], np.uint8).reshape(n, 3)
    return rec


SERVICES = [("Radio One", 0xC221, 3, 0, 3, 64, 0), ("Jazz 24", 0xC222, 7, 0, 2, 48, 48), ("News", 0xC223, 9, 1, 2, 32, 200)]
DAB_SERVICES = [("Classic", 0xC332, 11, 17, 100)]                            # UEP index 17: 64 kbit/s, 58 CUs


@pytest.fixture(scope="module")
def service_chain(ectx):
    """synth.ServiceEnsemble (3 DAB+ services + 1 UEP DAB service), 20 frames played once on a clean channel, through the
    front end: soft bits on the device, and the stream list in an order that is not the frame's."""
    import torch
    ens = synth.ServiceEnsemble(7, SERVICES, n_frames=20, dab_services=DAB_SERVICES, extras=False)   # four services fill the FIBs
    iq = ens.iq()
    soft, _, _ = ectx.ofdm_demod_frames(np.ascontiguousarray(iq[:, synth.NB_NULL:]), np.zeros(20, np.float32))
    scs = {3: dabgpu.subchannel(0, 64, level=3), 7: dabgpu.subchannel(48, 48, level=2),
           9: dabgpu.subchannel(200, 32, level=2, eep_type=1), 11: dabgpu.uep_subchannel(17, 100)}
    streams = [(9, scs[9]), (3, scs[3]), (11, scs[11]), (7, scs[7])]
    sent = {3: ens.msc_bytes[0], 7: ens.msc_bytes[1], 9: ens.msc_bytes[2], 11: ens.mp2_frames[0]}
    return ens, torch.from_numpy(soft).cuda(), streams, sent


@pytest.mark.gpu
def test_whole_chain_frames_equal_the_reference_writers(ectx, service_chain):
    """Case 6: every non-warm-up frame equals the reference writer's frame made from the TRANSMITTED FIBs and sub-channel
    bytes of CIF t - 15; frames 0..14 are warm-up frames."""
    ens, soft, streams, sent = service_chain
    eti, status, _ = ectx.decode_frames_eti(soft, 1, streams)
    eti = eti.cpu().numpy()[0]
    status = status.cpu().numpy().view(dabgpu.ETI_STATUS_DTYPE).reshape(-1)
    ref = [ref_stream(i, sc) for i, sc in streams]
    fibs = ens.fibs.reshape(80, 3, 32)
    assert eti.shape == (80, 6144)
    for t in range(80):
        c = t - 15
        info = dabgpu.eti_parse(eti[t])
        if c < 0:
            assert info["err"] == 0x00 and not info["fic"].any() and status[t]["flags"] == dabgpu.ETI_WARMUP and status[t]["fib_ok"] == 0
            assert status[t]["cif_count"] == (c % 5000) and info["fct"] == (c % 5000) % 250
            continue
        want = R.write_frame(ref, c, fibs[c].tobytes(), {i: sent[i][c] for i in sent}, 0xFF)
        assert eti[t].tobytes() == want, t
        own = R.fig0_0_count(info["fic"][:32], 1)
        assert own == c and info["fct"] == own % 250 and status[t]["cif_count"] == c and status[t]["flags"] == 0
        assert status[t]["fib_ok"] == 7 and status[t]["length"] == info["length"]


@pytest.mark.gpu
def test_two_calls_with_history_equal_one(ectx, service_chain):
    """Case 7."""
    ens, soft, streams, _ = service_chain
    one, st_one, _ = ectx.decode_frames_eti(soft, 1, streams)
    a, st_a, hist = ectx.decode_frames_eti(soft[:8], 1, streams)
    b, st_b, _ = ectx.decode_frames_eti(soft[8:], 1, streams, history=hist)
    import torch
    assert torch.equal(torch.cat([a, b], 1), one) and torch.equal(torch.cat([st_a, st_b], 1), st_one)
    st_b = st_b.cpu().numpy().view(dabgpu.ETI_STATUS_DTYPE).reshape(-1)
    assert not (st_b["flags"] & dabgpu.ETI_WARMUP).any() and len(st_b) == 48


@pytest.mark.gpu
def test_64_streams_are_independent_and_counts_wrap(ectx):
    """Case 8: 64 streams x 16 frames, every stream its own seed; start counts chosen so that the lower count wraps
    249 -> 0 and the whole count 4999 -> 0 inside the call."""
    rng = np.random.default_rng(8)
    streams = CONFIGS["uep_and_eep_b"]()
    starts = [(230 if s % 2 == 0 else 4970) + s for s in range(64)]
    fib, ok, outs = make_case(rng, streams, 64, 64, starts)
    eti, status, hist = run_eti(ectx, streams, fib, ok, outs)
    check_against_reference(streams, fib, ok, outs, eti, status, hist_out=hist)
    for s in (0, 1):
        counts = status[s]["cif_count"].astype(int)
        assert list(counts) == [(starts[s] - 15 + t) % 5000 for t in range(64)]
    assert 249 in status[0]["cif_count"] % 250 and 0 in status[1]["cif_count"] and 4999 in status[1]["cif_count"]


@pytest.mark.gpu
def test_damaged_fic(ectx):
    """Case 9: CIFs whose FIBs failed their CRC carry ERR = 0xE1 and FIB_CRC, the count stays anchored and continuous and
    both CRCs of the frame hold; a stream without one valid first FIB has no anchor and counts from 0 -- or from its
    history."""
    rng = np.random.default_rng(9)
    streams = CONFIGS["one_eep_a"]()
    fib, ok, outs = make_case(rng, streams, 3, 48, [100, 200, 300])
    bad = [0, 1, 2, 3, 17, 30]                              # stream 0: the first frame's four CIFs (so the anchor is CIF 4) and two more
    for c in bad:
        fib[0, c] = rng.integers(0, 256, (3, 32), dtype=np.uint8)
        ok[0, c] = 0
    fib[0, 20, 1, 5] ^= 0x10                                # one FIB of three
    ok[0, 20, 1] = 0
    fib[1, :, 0] = rng.integers(0, 256, (48, 32), dtype=np.uint8)      # stream 1: every first FIB bad
    ok[1, :, 0] = 0
    eti, status, hist = run_eti(ectx, streams, fib, ok, outs)
    check_against_reference(streams, fib, ok, outs, eti, status, hist_out=hist)
    for c in bad + [20]:
        info = dabgpu.eti_parse(eti[0, c + 15]) if c + 15 < 48 else None
        if info:
            assert info["err"] == 0xE1 and status[0, c + 15]["flags"] & dabgpu.ETI_FIB_CRC
    assert status[0, 35]["fib_ok"] == 0b101
    assert list(status[0]["cif_count"]) == [(100 - 15 + t) % 5000 for t in range(48)]
    assert (status[1]["flags"] & dabgpu.ETI_NO_ANCHOR).all() and list(status[1]["cif_count"][15:18]) == [0, 1, 2]
    assert not (status[2]["flags"] & dabgpu.ETI_NO_ANCHOR).any()
    # the same streams continued: stream 1 still without an anchor goes on from its history (48, 49, ...)
    fib2, ok2, outs2 = make_case(rng, streams, 3, 16, [148, 248, 348])
    fib2[1, :, 0, 0] ^= 0xFF
    ok2[1, :, 0] = 0
    eti2, status2, hist2 = run_eti(ectx, streams, fib2, ok2, outs2, history=hist)
    ref_h = check_against_reference(streams, fib, ok, outs, eti, status)
    check_against_reference(streams, fib2, ok2, outs2, eti2, status2, history=ref_h, hist_out=hist2)
    assert list(status2[1]["cif_count"]) == [(48 - 15 + t) for t in range(16)] and (status2[1]["flags"] & dabgpu.ETI_NO_ANCHOR).all()
    assert not (status2["flags"] & dabgpu.ETI_WARMUP).any()


@pytest.mark.gpu
def test_start_override_and_spliced_stream(ectx):
    """Case 10."""
    rng = np.random.default_rng(10)
    streams = CONFIGS["uep_and_eep_b"]()
    fib, ok, outs = make_case(rng, streams, 3, 40, [10, 10, 10])
    # stream 1: the second half comes from an ensemble whose count is elsewhere
    other, _, _ = make_case(rng, streams, 1, 40, [3000])
    fib[1, 20:] = other[0, 20:]
    eti, status, _ = run_eti(ectx, streams, fib, ok, outs)
    check_against_reference(streams, fib, ok, outs, eti, status)
    mism = (status["flags"] & dabgpu.ETI_COUNT_MISMATCH) != 0
    assert not mism[0].any() and not mism[2].any()
    assert list(np.nonzero(mism[1])[0]) == list(range(35, 40))          # CIFs 20.. arrive in frames 35..
    assert list(status[1]["cif_count"]) == [(10 - 15 + t) % 5000 for t in range(40)]
    # the caller's own start counts: stream 0 overridden (every own count then disagrees), stream 1 left alone (-1), stream 2
    # overridden with what the FIC says anyway
    start = [4990, -1, 10]
    eti, status, _ = run_eti(ectx, streams, fib, ok, outs, cif_start=start)
    check_against_reference(streams, fib, ok, outs, eti, status, cif_start=start)
    assert list(status[0]["cif_count"]) == [(4990 - 15 + t) % 5000 for t in range(40)]
    assert ((status[0, 15:]["flags"] & dabgpu.ETI_COUNT_MISMATCH) != 0).all() and status[2]["flags"][15:].max() == 0


@pytest.mark.gpu
def test_reading_back_from_the_eti_bytes_alone(ectx, service_chain):
    """Case 11: eti_parse + the FIG oracle recover the sub-channel table equal to the frames' own STC, and the DAB+
    decoder finds the transmitted access units in a stream taken out of the frames."""
    from oracle import fig_oracle as FO
    ens, soft, streams, _ = service_chain
    eti, status, _ = ectx.decode_frames_eti(soft, 1, streams)
    frames = [dabgpu.eti_parse(f) for f in eti.cpu().numpy()[0][15:]]
    db = FO.parse_fibs(np.concatenate([f["fic"] for f in frames]).reshape(-1, 32))
    table = sorted(l for l in db.lines() if l.startswith("subchannel "))
    stc = frames[0]["streams"]
    assert all([(s["scid"], s["sad"], s["tpl"], s["stl"]) for s in f["streams"]] == [(s["scid"], s["sad"], s["tpl"], s["stl"]) for s in stc]
               for f in frames)
    assert len(table) == len(stc) == 4
    by_id = {int(re.match(r"subchannel id=(\d+) ", l).group(1)): dict(kv.split("=") for kv in l.split()[1:]) for l in table}
    for s in stc:
        row = by_id[s["scid"]]
        assert int(row["start"]) == s["sad"]
        if int(row["uep"]):                                         # short form: size, rate and level from the table index
            sc = dabgpu.uep_subchannel(int(row["uep_index"]), s["sad"])
            assert s["tpl"] == 0x10 | (sc.protection_level - 1)
        else:
            sc = dabgpu.Subchannel(s["sad"], int(row["length"]), 0, int(row["eep_type"]), int(row["eep_level"]) + 1, s["stl"] * 8 // 3)
            assert s["tpl"] == 0x20 | (sc.eep_type << 2) | (sc.protection_level - 1)
        # the sizes the FIC announces are the sizes of sub-channels of the STC's bit rates
        assert dabgpu.lib().dabgpu_subchannel_bytes(C.byref(sc)) == 8 * s["stl"]
        assert [x.length for _, x in streams if x.start_address == s["sad"]] == [sc.length]
    # sub-channel 3 (64 kbit/s DAB+): CIFs 0..64 -> 13 super-frames of 5 logical frames
    k = [s["scid"] for s in stc].index(3)
    assert stc[k]["stl"] * 8 == 192
    lf = np.stack([f["streams"][k]["data"] for f in frames])
    out, st = ectx.dabplus_superframes(lf.reshape(13, 960), 64)
    assert st["firecode_ok"].all() and (st["rs_uncorrectable"] == 0).all()
    for n in range(13):
        aus = ens.aus[0][n % len(ens.aus[0])]
        assert st[n]["num_aus"] == len(aus)
        for a, au in enumerate(aus):
            got = out[n, st[n]["au_start"][a]:st[n]["au_start"][a + 1]]
            assert got.tobytes() == np.asarray(au, np.uint8).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_streams,n_frames", [("one_eep_a", 1, 1), ("tiny", 2, 3), ("full_cif", 2, 5), ("fic_only", 1, 4),
                                                     ("multiplex18", 3, 8)])
def test_odd_shapes(ectx, name, n_streams, n_frames):
    """Case 12, and the multiplex of the timing: calls shorter than the FIC delay, the smallest and the largest sub-channel."""
    rng = np.random.default_rng(12)
    streams = CONFIGS[name]()
    n_cif = 4 * n_frames
    fib, ok, outs = make_case(rng, streams, n_streams, n_cif, [4990 + 7 * s for s in range(n_streams)])
    eti, status, hist = run_eti(ectx, streams, fib, ok, outs)
    ref_h = check_against_reference(streams, fib, ok, outs, eti, status, hist_out=hist)
    # ... continued twice: a history of fewer than 15 CIFs is carried on
    for _ in range(2):
        fib2, ok2, outs2 = make_case(rng, streams, n_streams, n_cif, [int(h["next_count"]) for h in ref_h])
        eti2, status2, hist2 = run_eti(ectx, streams, fib2, ok2, outs2, history=hist)
        ref_h = check_against_reference(streams, fib2, ok2, outs2, eti2, status2, history=ref_h, hist_out=hist2)
        hist = hist2


@pytest.mark.gpu
def test_refused_calls_enqueue_nothing(ectx):
    import torch
    streams = CONFIGS["one_eep_a"]()
    plan = dabgpu.eti_layout(streams)
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")
    fib, ok, out, eti, st, h = z(4, 12, 32), z(4, 12), z(1, 16, 192), z(1, 16, 6144), z(1, 16, 8), z(1, 1504)
    args = lambda **kw: dict(dict(plan=plan, n_streams=1, frames_per_stream=4, d_fib=fib.data_ptr(), d_crc_ok=ok.data_ptr(),
                                  d_out=[out.data_ptr()], d_eti=eti.data_ptr(), d_status=st.data_ptr()), **kw)
    bad_plan = dabgpu.eti_layout(streams)
    bad_plan.bytes[0] = 200
    for kw in (dict(d_eti=eti.data_ptr() + 8), dict(d_out=[out.data_ptr() + 4]), dict(plan=bad_plan), dict(n_streams=-1),
               dict(d_history_in=h.data_ptr(), d_history_out=h.data_ptr()), dict(d_status=st.data_ptr() + 4)):
        with pytest.raises(dabgpu.DabGpuError) as e:
            ectx.eti_frames_dev(**args(**kw))
        assert e.value.status == -1
    ectx.sync()
    assert not eti.any() and not st.any()
    ectx.set_timing(True)
    ectx.eti_frames_dev(**args())
    assert ectx.last_kernel_ms(7) > 0 and ectx.mean_kernel_ms(7)[1] == 1
    ectx.set_timing(False)
