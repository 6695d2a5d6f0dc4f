"""The launch path the entry-table calls share (csrc/dabgpu_ctx.hpp: stage_table, launch_entry_table): a call's device table lives
in a staging slot of the context that is freed and allocated again when a call needs more than it holds -- which must not happen
under a launch that still reads it.  Three calls whose tables differ in kind -- pad_labels_dev (entries of one size),
eti_read_dev (scratch per entry behind the table), packet_groups_dev (two tables and scan records) -- each run with 1 entry, then
70, then 1 again on ONE context and ONE stream that is not the context's own, with no host synchronisation of the test's between
the three; every byte of every run's memory (outputs, and what must stay as it was) is then compared with the call's host twin
on the same image.  Inputs are as small as the tests of those calls use."""
import ctypes as C

import numpy as np
import pytest

import dabgpu
import test_eti_read as TE
import test_packet_groups as TG
import test_pad_labels as TP
from dabgpu import synth
from test_eti import CONFIGS

FILL = 0xEE
COUNTS = (1, 70, 1)


class Layout:
    """Regions of one allocation, each on a 256-byte boundary with FILL before, behind and inside it unless `data` is given."""

    def __init__(self):
        self.size, self.parts = 0, []

    def take(self, n, data=None):
        off = (self.size + 64 + 255) // 256 * 256
        self.size = off + n
        if data is not None:
            self.parts.append((off, np.frombuffer(bytes(data), np.uint8)))
        return off

    def image(self):
        img = np.full(self.size + 64, FILL, np.uint8)
        for off, d in self.parts:
            img[off:off + d.size] = d
        return img


# ------------------------------------------------------------------ the three calls: n entries -> (layout, base -> entries)
def pad_entries(n, seed):
    """n DAB+ services at 64 kbit/s, two or three super-frames each, every one with a label of its own"""
    lay, regions = Layout(), []
    nb = dabgpu.pad_state_bytes()
    for e in range(n):
        text = b"run %d entry %d" % (seed, e)
        data, status = TP.superframes(100 * seed + e, 8, 3, TP.var(TP.label(text, e & 1), 2 + e % 3))
        follow = np.zeros(1, dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)
        follow["n_superframes"], follow["synced"] = len(data), 1
        regions.append((lay.take(data.size, data.tobytes()), lay.take(64 * len(data), status.tobytes()), lay.take(32, follow.tobytes()), len(data),
                        lay.take(nb), lay.take(144), lay.take(64)))

    def at(base):
        return [dabgpu.PadEntry(d_data=base + d, data_stride=880, d_status=base + st, d_follow=base + fo, bitrate_kbps=64, max_superframes=rows,
                                d_state_in=None, d_state_out=base + so, d_label=base + la, d_result=base + re)
                for d, st, fo, rows, so, la, re in regions], None
    return lay, at


_ETI_STREAMS = {}


def eti_entries(n, seed):
    """n ETI(NI) byte streams of three frames, of two configurations, each beginning at another byte of its first frame"""
    lay, regions = Layout(), []
    for e in range(n):
        name = ("tiny", "uep_and_eep_b")[e % 2]
        if name not in _ETI_STREAMS:
            _ETI_STREAMS[name] = b"".join(TE.make_frames(name, 3, 50)[0])
        case = TE.Case(CONFIGS[name](), _ETI_STREAMS[name][(17 * (e + seed)) % 6144 if e else 0:])
        rows = max(case.rows, 1)
        regions.append((case, lay.take(len(case.data), case.data), lay.take(TE.STATE_BYTES), lay.take(rows * 96), lay.take(rows * 3),
                        lay.take(rows * 16), lay.take(48), [lay.take(rows * k) for k in case.sizes]))

    def at(base):
        entries, keep = [], []
        for case, by, so, fib, ok, st, re, outs in regions:
            ptrs = (C.c_void_p * len(outs))(*[base + o for o in outs])
            keep += [ptrs, case]
            entries.append(dabgpu.EtiReadEntry(d_bytes=base + by, n_bytes=len(case.data), plan=C.pointer(case.plan),
                                               d_out=C.cast(ptrs, C.POINTER(C.c_void_p)), d_state_in=None, d_state_out=base + so, d_fib=base + fib,
                                               d_crc_ok=base + ok, d_status=base + st, d_result=base + re))
        return entries, keep
    return lay, at


N_CIFS = 4


def groups_entries(n, seed):
    """n packet-mode components at 64 kbit/s, four frames each, three data groups of its own lengths in every one"""
    lay, regions = Layout(), []
    nb, rb = dabgpu.packet_groups_state_bytes(), dabgpu.PACKET_GROUPS_RESULT_DTYPE.itemsize
    for e in range(n):
        groups = [synth.msc_data_group(k, TG.payload(20 + e % 23 + 7 * k, 1000 * seed + 10 * e + k), continuity=k + 1) for k in range(3)]
        frames = TG.frames_of(64, synth.packetise(groups, TG.ADDR, (2,), 0), N_CIFS)
        assert frames.shape == (N_CIFS, 192)
        regions.append((lay.take(frames.size, frames.tobytes()), e % 2, lay.take(nb), lay.take(1024), lay.take(16 * 32), lay.take(rb)))

    def at(base):
        return [dabgpu.PacketGroupsEntry(d_in=base + fr, in_stride=192, bitrate_kbps=64, address=TG.ADDR, fec=0, mode=mode, keep_repeats=0,
                                         d_state_in=None, d_state_out=base + so, d_bytes=base + by, d_groups=base + gr, bytes_capacity=1024,
                                         max_groups=16, d_result=base + re)
                for fr, mode, so, by, gr, re in regions], None
    return lay, at


KINDS = {"pad_labels": (pad_entries, dabgpu.pad_labels_host, "pad_labels_dev", ()),
         "eti_read": (eti_entries, dabgpu.eti_read_host, "eti_read_dev", ()),
         "packet_groups": (groups_entries, dabgpu.packet_groups_host, "packet_groups_dev", (N_CIFS,))}


def host_run(kind, n, seed):
    """-> (the image before, the image after the host twin)"""
    build, host, _, args = KINDS[kind]
    lay, at = build(n, seed)
    img = lay.image()
    buf = TE.aligned(img.size)
    buf[:] = img
    entries, keep = at(buf.ctypes.data)
    host(entries, *args)
    return img, buf, at


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_host_twins_write_something_per_entry(built, kind):
    """what the GPU test compares with is not an image nobody wrote to: every entry's result record is written, runs differ"""
    img, after, _ = host_run(kind, max(COUNTS), 1)
    assert not np.array_equal(img, after)
    assert not np.array_equal(after, host_run(kind, max(COUNTS), 2)[1])


@pytest.fixture(scope="module")
def one_context_one_stream(built):
    import torch
    from conftest import make_ctx
    c = make_ctx()
    yield c, torch.cuda.Stream()
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_gpu_the_table_grows_between_launches_on_one_stream(one_context_one_stream, kind):
    import torch
    ctx, stream = one_context_one_stream
    _, _, dev, args = KINDS[kind]
    runs = []
    for seed, n in enumerate(COUNTS):
        img, want, at = host_run(kind, n, seed)
        runs.append((torch.from_numpy(img).cuda(), want, at))
    # 1 entry; 70, so that the slot grows while the first launch may still be in flight; 1 again.  The test waits once, at the end.
    for t, _, at in runs:
        entries, keep = at(t.data_ptr())
        assert t.data_ptr() % 256 == 0
        getattr(ctx, dev)(entries, *args, stream=stream.cuda_stream)
    stream.synchronize()
    for (t, want, _), n in zip(runs, COUNTS):
        got = t.cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s with %d entries: %d bytes differ from the host twin's, the first at %s" % (kind, n, bad.size, bad[:8])
