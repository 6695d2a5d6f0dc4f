"""Device time of the EDI writer and reader (dabgpu_edi_frames_dev, dabgpu_edi_read_dev) beside the ETI(NI) writer and reader
on the same 64 ensembles of the 18-sub-channel multiplex (tools/eti_read_time.py's shapes: 16 and 256 transmission frames per
ensemble and call), in interleaved rounds of one run: every round times the four calls at both shapes once, with events on
the context's stream; the medians over the rounds are printed.  The EDI reader's host call runs once per shape.

  python tools/edi_time.py [--streams 64] [--rounds 9] [--no-host]

The packets are the writer's own output (random FIBs and sub-channel bytes: every packet is a row); one JSON line at the end."""
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
from eti_read_time import Shape  # noqa: E402
from eti_timing import multiplex18  # noqa: E402


class EdiShape(Shape):
    """the ETI shape, and the same decode buffers written and read as EDI"""

    def __init__(self, ctx, E, F, scs, plan, dev):
        super().__init__(ctx, E, F, scs, plan, dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        n_cif = self.n_cif
        self.packet = dabgpu.edi_packet_bytes(plan)
        self.stride = (n_cif * self.packet + 15) // 16 * 16
        self.rows = dabgpu.edi_read_max_rows(n_cif * self.packet, plan)
        self.edi = torch.zeros((E, self.stride), **u8)
        self.e_wstatus = torch.empty((E, n_cif, 8), **u8)
        self.e_fib, self.e_ok = torch.empty((E, self.rows, 96), **u8), torch.empty((E, self.rows, 3), **u8)
        self.e_outs = [torch.empty((E, self.rows, sc.bitrate_kbps * 3), **u8) for sc in scs]
        self.e_status, self.e_result = torch.empty((E, self.rows, 32), **u8), torch.empty((E, 48), **u8)
        self.e_state = torch.empty((E, dabgpu.edi_read_state_bytes()), **u8)
        self.e_entries = []
        for s in range(E):
            ptrs = (C.c_void_p * len(scs))(*[o[s].data_ptr() for o in self.e_outs])
            self.keep.append(ptrs)
            self.e_entries.append(dabgpu.EdiReadEntry(self.edi[s].data_ptr(), n_cif * self.packet, 0, C.pointer(plan),
                                                      C.cast(ptrs, C.POINTER(C.c_void_p)), None, self.e_state[s].data_ptr(),
                                                      self.e_fib[s].data_ptr(), self.e_ok[s].data_ptr(), self.e_status[s].data_ptr(),
                                                      self.e_result[s].data_ptr()))

    def edi_write(self, s):
        self.ctx.edi_frames_dev(self.plan, self.E, self.F, self.fib.data_ptr(), self.ok.data_ptr(), [o.data_ptr() for o in self.outs],
                                self.edi.data_ptr(), self.stride, self.e_wstatus.data_ptr(), d_history_out=self.hist.data_ptr(), stream=s)

    def edi_read(self, s):
        self.ctx.edi_read_dev(self.e_entries, stream=s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    scs = multiplex18()
    plan = dabgpu.eti_layout([(i, sc) for i, sc in enumerate(scs)])
    E = a.streams
    ctx = dabgpu.Context(device=0, max_frames=E * 256)
    s = ctx.stream
    ext = torch.cuda.ExternalStream(s)
    shapes = {F: EdiShape(ctx, E, F, scs, plan, dev) for F in (16, 256)}
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext)
        fn(s)
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1)

    calls = ("eti_write", "eti_read", "edi_write", "edi_read")
    fns = lambda sh: dict(eti_write=sh.write, eti_read=sh.read, edi_write=sh.edi_write, edi_read=sh.edi_read)
    for sh in shapes.values():                                # warm-up: frames and packets exist, the stage areas have their size
        for _ in range(2):
            for what in calls:
                fns(sh)[what](s)
    ctx.sync()
    ms = {(what, F): [] for what in calls for F in shapes}
    for _ in range(a.rounds):
        for F, sh in shapes.items():
            for what in calls:
                ms[(what, F)].append(timed(fns(sh)[what]))
    row = {"ensembles": E, "rounds": a.rounds}
    for F, sh in shapes.items():
        res = sh.e_result.cpu().numpy().view(dabgpu.EDI_READ_RESULT_DTYPE).reshape(-1)
        assert (res["rows"] == sh.n_cif).all() and not res["skipped"].any() and not res["tail_bytes"].any(), res[:2]
        assert all(torch.equal(x, y[:, :sh.n_cif]) for x, y in zip(sh.outs, sh.e_outs)), "the reader's rows are not the writer's"
        med = {what: float(np.median(ms[(what, F)])) for what in calls}
        cifs = E * sh.n_cif
        edi_bytes = cifs * sh.packet
        row["F%d" % F] = dict({k + "_ms": v for k, v in med.items()}, cifs=cifs, packet_bytes=sh.packet, edi_bytes=edi_bytes,
                              edi_read_over_eti_read=med["edi_read"] / med["eti_read"], edi_write_over_eti_write=med["edi_write"] / med["eti_write"],
                              all={k: ms[(k, F)] for k in calls})
        print("%4d frames x %d ensembles = %6d CIFs: ETI writer %.4f ms, EDI writer %.4f ms (%.2f x); ETI reader %.4f ms, EDI reader %.4f ms "
              "(%.2f x), %d-byte packets, %.1f MB of EDI, %.0f GB/s in" % (F, E, cifs, med["eti_write"], med["edi_write"],
                                                                           med["edi_write"] / med["eti_write"], med["eti_read"], med["edi_read"],
                                                                           med["edi_read"] / med["eti_read"], sh.packet, edi_bytes / 1e6,
                                                                           edi_bytes / med["edi_read"] / 1e6))
        if not a.no_host:
            edi_h = sh.edi.cpu().numpy()
            fib_h, ok_h = np.empty((E, sh.rows, 96), np.uint8), np.empty((E, sh.rows, 3), np.uint8)
            outs_h = [np.empty((E, sh.rows, sc.bitrate_kbps * 3), np.uint8) for sc in scs]
            st_h, res_h = np.empty((E, sh.rows, 32), np.uint8), np.empty((E, 48), np.uint8)
            state_h = np.empty((E, dabgpu.edi_read_state_bytes() + 16), np.uint8)
            keep, entries = [], []
            for k in range(E):
                ptrs = (C.c_void_p * len(scs))(*[o[k].ctypes.data for o in outs_h])
                keep.append(ptrs)
                so = state_h[k].ctypes.data
                entries.append(dabgpu.EdiReadEntry(edi_h[k].ctypes.data, sh.n_cif * sh.packet, 0, C.pointer(plan), C.cast(ptrs, C.POINTER(C.c_void_p)),
                                                   None, so + (-so) % 16, fib_h[k].ctypes.data, ok_h[k].ctypes.data, st_h[k].ctypes.data,
                                                   res_h[k].ctypes.data))
            t0 = time.perf_counter()
            dabgpu.edi_read_host(entries)
            host_ms = 1e3 * (time.perf_counter() - t0)
            assert all(np.array_equal(x[:, :sh.n_cif], y.cpu().numpy()[:, :sh.n_cif]) for x, y in zip(outs_h, sh.e_outs))
            row["F%d" % F].update(host_ms=host_ms, host_over_device=host_ms / med["edi_read"])
            print("     EDI host call, one thread, the same packets: %.1f ms (%.0f x the device call)" % (host_ms, host_ms / med["edi_read"]))
    ctx.close()
    print(json.dumps(row))


if __name__ == "__main__":
    main()
