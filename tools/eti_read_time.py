"""Device time of the ETI(NI) reader (dabgpu_eti_read_dev: scan, chain, rows, finish) beside the writer of the same
frames (dabgpu_eti_frames_dev) and the reader's host twin (dabgpu_eti_read_host), for the 64 ensembles of the
18-sub-channel multiplex of tools/eti_timing.py at 16 and at 256 transmission frames (64 and 1024 ETI frames) per ensemble
and call.  One run, interleaved rounds: every round times writer and reader at both shapes once, with events on the
context's stream; the medians over the rounds are printed.  The host twin runs once per shape on the downloaded frames.

  python tools/eti_read_time.py [--streams 64] [--rounds 9] [--no-host]

The frames are the writer's own output (random FIBs and sub-channel bytes: the work does not depend on the values, every
frame is taken); one JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dabgpu  # noqa: E402
from eti_timing import multiplex18  # noqa: E402


class Shape:
    def __init__(self, ctx, E, F, scs, plan, dev):
        u8 = dict(dtype=torch.uint8, device=dev)
        self.E, self.F, self.n_cif = E, F, 4 * F
        n_cif = self.n_cif
        self.fib = torch.randint(0, 256, (E * F, 12, 32), **u8)
        self.ok = torch.ones((E * F, 12), **u8)
        self.outs = [torch.randint(0, 256, (E, n_cif, sc.bitrate_kbps * 3), **u8) for sc in scs]
        self.eti = torch.empty((E, n_cif, dabgpu.ETI_FRAME_BYTES), **u8)
        self.wstatus = torch.empty((E, n_cif, 8), **u8)
        self.hist = torch.zeros((E, dabgpu.eti_history_bytes()), **u8)
        # the reader's side
        self.r_fib, self.r_ok = torch.empty((E, n_cif, 96), **u8), torch.empty((E, n_cif, 3), **u8)
        self.r_outs = [torch.empty((E, n_cif, sc.bitrate_kbps * 3), **u8) for sc in scs]
        self.r_status, self.r_result = torch.empty((E, n_cif, 16), **u8), torch.empty((E, 48), **u8)
        self.r_state = torch.empty((E, dabgpu.eti_read_state_bytes()), **u8)
        self.keep, self.entries = [], []
        for s in range(E):
            ptrs = (C.c_void_p * len(scs))(*[o[s].data_ptr() for o in self.r_outs])
            self.keep.append(ptrs)
            self.entries.append(dabgpu.EtiReadEntry(self.eti[s].data_ptr(), n_cif * dabgpu.ETI_FRAME_BYTES, 0, C.pointer(plan),
                                                    C.cast(ptrs, C.POINTER(C.c_void_p)), None, self.r_state[s].data_ptr(), self.r_fib[s].data_ptr(),
                                                    self.r_ok[s].data_ptr(), self.r_status[s].data_ptr(), self.r_result[s].data_ptr()))
        self.ctx, self.plan = ctx, plan

    def write(self, s):
        self.ctx.eti_frames_dev(self.plan, self.E, self.F, self.fib.data_ptr(), self.ok.data_ptr(), [o.data_ptr() for o in self.outs],
                                self.eti.data_ptr(), self.wstatus.data_ptr(), d_history_out=self.hist.data_ptr(), stream=s)

    def read(self, s):
        self.ctx.eti_read_dev(self.entries, stream=s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    scs = multiplex18()
    streams = [(i, sc) for i, sc in enumerate(scs)]
    plan = dabgpu.eti_layout(streams)
    E = a.streams
    ctx = dabgpu.Context(device=0, max_frames=E * 256)
    s = ctx.stream
    ext = torch.cuda.ExternalStream(s)
    shapes = {F: Shape(ctx, E, F, scs, plan, dev) for F in (16, 256)}
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext)
        fn(s)
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for sh in shapes.values():                                # warm-up: the frames exist, the tables have their size
        for _ in range(2):
            sh.write(s)
            sh.read(s)
    ctx.sync()
    ms = {(what, F): [] for what in ("write", "read") for F in shapes}
    for _ in range(a.rounds):
        for F, sh in shapes.items():
            ms[("write", F)].append(timed(sh.write))
            ms[("read", F)].append(timed(sh.read))
    row = {"ensembles": E, "rounds": a.rounds}
    for F, sh in shapes.items():
        res = sh.r_result.cpu().numpy().view(dabgpu.ETI_READ_RESULT_DTYPE).reshape(-1)
        assert (res["taken"] == sh.n_cif).all() and not res["skipped"].any(), res[:2]
        assert all(torch.equal(x, y) for x, y in zip(sh.outs, sh.r_outs)), "the reader's rows are not the writer's"
        w, r = float(np.median(ms[("write", F)])), float(np.median(ms[("read", F)]))
        frames = E * sh.n_cif
        read_bytes = frames * 6144
        out_bytes = sh.r_fib.numel() + sh.r_ok.numel() + sh.r_status.numel() + sum(o.numel() for o in sh.r_outs)
        row["F%d" % F] = {"eti_frames": frames, "write_ms": w, "read_ms": r, "read_over_write": r / w, "read_us_per_frame": 1e3 * r / frames,
                          "read_GBps_in": read_bytes / r / 1e6, "bytes_in": read_bytes, "bytes_out": out_bytes,
                          "write_ms_all": ms[("write", F)], "read_ms_all": ms[("read", F)]}
        print("%4d frames x %d ensembles = %6d ETI frames (%.1f MB): writer median %.4f ms, reader median %.4f ms (%.2f x the writer), "
              "%.3f us per frame, %.0f GB/s of frames in" % (F, E, frames, read_bytes / 1e6, w, r, r / w, 1e3 * r / frames, read_bytes / r / 1e6))
        if not a.no_host:
            eti_h = sh.eti.cpu().numpy()
            fib_h, ok_h = np.empty((E, sh.n_cif, 96), np.uint8), np.empty((E, sh.n_cif, 3), np.uint8)
            outs_h = [np.empty((E, sh.n_cif, sc.bitrate_kbps * 3), np.uint8) for sc in scs]
            st_h, res_h = np.empty((E, sh.n_cif, 16), np.uint8), np.empty((E, 48), np.uint8)
            state_h = np.empty((E, dabgpu.eti_read_state_bytes() + 16), np.uint8)
            keep, entries = [], []
            for k in range(E):
                ptrs = (C.c_void_p * len(scs))(*[o[k].ctypes.data for o in outs_h])
                keep.append(ptrs)
                so = state_h[k].ctypes.data
                entries.append(dabgpu.EtiReadEntry(eti_h[k].ctypes.data, sh.n_cif * 6144, 0, C.pointer(plan), C.cast(ptrs, C.POINTER(C.c_void_p)),
                                                   None, so + (-so) % 16, fib_h[k].ctypes.data, ok_h[k].ctypes.data, st_h[k].ctypes.data,
                                                   res_h[k].ctypes.data))
            t0 = time.perf_counter()
            dabgpu.eti_read_host(entries)
            host_ms = 1e3 * (time.perf_counter() - t0)
            assert all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(outs_h, sh.r_outs))
            row["F%d" % F].update(host_ms=host_ms, host_over_device=host_ms / r)
            print("     host twin, one thread, the same frames: %.1f ms (%.0f x the device call)" % (host_ms, host_ms / r))
    ctx.close()
    print(json.dumps(row))


if __name__ == "__main__":
    main()
