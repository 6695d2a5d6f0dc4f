"""Device time of the PFT writer and reader (dabgpu_pft_fragments_dev, dabgpu_pft_read_dev) beside the EDI writer and reader on
the 64 ensembles of tools/edi_time.py (the 18-sub-channel multiplex, 16 and 256 transmission frames per ensemble and call),
in interleaved rounds of one run: every round times the five calls at both shapes once, with events on the context's stream;
the medians over the rounds are printed.  The reader is timed on every packet's whole fragment set and on a stream from which
guaranteed_losses fragments of every packet are missing (every chunk of every packet is then filled).  The host twins run once,
at the 16-frame shape.

  python tools/pft_time.py [--streams 64] [--rounds 9] [--m 2] [--no-host]

The AF packets are the EDI writer's own output; what the readers give back is held to them.  One JSON line at the end."""
import argparse
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
from edi_time import EdiShape  # noqa: E402
from eti_timing import multiplex18  # noqa: E402


def pad16(n):
    return (n + 15) // 16 * 16


class PftShape(EdiShape):
    """the EDI shape, its packets cut into fragments, and two fragment streams read back"""

    def __init__(self, ctx, E, F, scs, plan, dev, m):
        super().__init__(ctx, E, F, scs, plan, dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        self.layout = lay = dabgpu.pft_layout(self.packet, True, m)
        self.n_pf = self.n_cif * lay.stream_bytes
        self.pf_stride = pad16(self.n_pf)
        self.pf = torch.zeros((E, self.pf_stride), **u8)
        self.pseq = [(977 * s) & 0xFFFF for s in range(E)]
        self.fb = lay.header_bytes + lay.plen
        self.n_lossy = self.n_cif * (lay.fcount - lay.guaranteed_losses) * self.fb
        self.lossy = torch.zeros((E, pad16(self.n_lossy)), **u8)
        self.sides = {}
        for name, src, n in (("whole", self.pf, self.n_pf), ("lossy", self.lossy, self.n_lossy)):
            out = torch.empty((E, dabgpu.pft_read_out_bytes(n)), **u8)
            rec = torch.empty((E, dabgpu.pft_read_max_records(n), 32), **u8)
            res, state = torch.empty((E, 64), **u8), torch.empty((E, dabgpu.pft_read_state_bytes()), **u8)
            entries = [dabgpu.PftReadEntry(src[s].data_ptr(), n, dabgpu.PFT_READ_FLUSH, None, state[s].data_ptr(), out[s].data_ptr(),
                                           rec[s].data_ptr(), res[s].data_ptr()) for s in range(E)]
            self.sides[name] = dict(out=out, rec=rec, res=res, state=state, entries=entries)

    def pft_write(self, s):
        self.ctx.pft_fragments_dev(self.layout, self.E, self.n_cif, self.edi.data_ptr(), self.stride, self.pf.data_ptr(), self.pf_stride,
                                   self.pseq, stream=s)

    def make_lossy(self):
        """the fragments of self.pf without guaranteed_losses of every packet's (another set for every packet)"""
        lay, E, n = self.layout, self.E, self.n_cif
        keep = lay.fcount - lay.guaranteed_losses
        rng = np.random.default_rng(self.F)
        picks = np.stack([np.sort(rng.permutation(lay.fcount)[:keep]) for _ in range(n)])            # [n][keep]
        index = torch.from_numpy((np.arange(n)[:, None] * lay.fcount + picks).reshape(-1)).to(self.pf.device)
        frags = self.pf[:, :self.n_pf].reshape(E, n * lay.fcount, self.fb)
        self.lossy[:, :self.n_lossy] = frags[:, index].reshape(E, -1)

    def pft_read(self, s):
        self.ctx.pft_read_dev(self.sides["whole"]["entries"], stream=s)

    def pft_read_lossy(self, s):
        self.ctx.pft_read_dev(self.sides["lossy"]["entries"], stream=s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    scs = multiplex18()
    plan = dabgpu.eti_layout([(i, sc) for i, sc in enumerate(scs)])
    E = a.streams
    ctx = dabgpu.Context(device=0, max_frames=E * 256)
    s = ctx.stream
    ext = torch.cuda.ExternalStream(s)
    shapes = {F: PftShape(ctx, E, F, scs, plan, dev, a.m) for F in (16, 256)}
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext)
        fn(s)
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1)

    calls = ("edi_write", "edi_read", "pft_write", "pft_read", "pft_read_lossy")
    fns = lambda sh: dict(edi_write=sh.edi_write, edi_read=sh.edi_read, pft_write=sh.pft_write, pft_read=sh.pft_read,
                          pft_read_lossy=sh.pft_read_lossy)
    for sh in shapes.values():                                # warm-up: packets and fragments exist, the stage areas have their size
        sh.write(s)                                           # (the ETI writer leaves the history the EDI writer starts from)
        sh.edi_write(s)
        sh.pft_write(s)
        ctx.sync()
        sh.make_lossy()
        torch.cuda.synchronize()
        for _ in range(2):
            for what in calls:
                fns(sh)[what](s)
    ctx.sync()
    ms = {(what, F): [] for what in calls for F in shapes}
    for _ in range(a.rounds):
        for F, sh in shapes.items():
            for what in calls:
                ms[(what, F)].append(timed(fns(sh)[what]))
    row = {"ensembles": E, "rounds": a.rounds, "m": a.m}
    for F, sh in shapes.items():
        lay, n_af = sh.layout, sh.n_cif * sh.packet
        for name, side in sh.sides.items():
            res = side["res"].cpu().numpy().view(dabgpu.PFT_READ_RESULT_DTYPE).reshape(-1)
            assert (res["packets"] == sh.n_cif).all() and (res["out_bytes"] == n_af).all() and not res["lost"].any() and not res["skipped"].any(), res[:2]
            assert (res["recovered"] == (sh.n_cif if name == "lossy" else 0)).all(), res[:2]
            assert torch.equal(side["out"][:, :n_af], sh.edi[:, :n_af]), "the PFT reader's packets are not the EDI writer's"
            rec = side["rec"][:, :sh.n_cif].cpu().numpy().view(dabgpu.PFT_READ_RECORD_DTYPE)
            assert (rec["flags"] & dabgpu.PFT_AF_OK).all()
        filled = int(sh.sides["lossy"]["res"].cpu().numpy().view(dabgpu.PFT_READ_RESULT_DTYPE)["chunks_filled"].sum())
        med = {what: float(np.median(ms[(what, F)])) for what in calls}
        cifs = E * sh.n_cif
        row["F%d" % F] = dict({k + "_ms": v for k, v in med.items()}, cifs=cifs, packet_bytes=sh.packet, chunks=lay.chunks, rs_k=lay.rs_k,
                              fcount=lay.fcount, plen=lay.plen, guaranteed_losses=lay.guaranteed_losses, pf_bytes=E * sh.n_pf,
                              chunks_filled=filled, pft_write_over_edi_write=med["pft_write"] / med["edi_write"],
                              pft_read_over_edi_read=med["pft_read"] / med["edi_read"],
                              pft_read_lossy_over_edi_read=med["pft_read_lossy"] / med["edi_read"], all={k: ms[(k, F)] for k in calls})
        print("%4d frames x %d ensembles = %6d packets of %d bytes (%d chunks, %d fragments of %d, any %d may be lost): EDI writer %.4f ms, PFT "
              "writer %.4f ms (%.2f x); EDI reader %.4f ms, PFT reader %.4f ms (%.2f x), with %d fragments of every packet missing %.4f ms "
              "(%.2f x; %d chunks filled), %.1f MB of fragments" %
              (F, E, cifs, sh.packet, lay.chunks, lay.fcount, lay.plen, lay.guaranteed_losses, med["edi_write"], med["pft_write"],
               med["pft_write"] / med["edi_write"], med["edi_read"], med["pft_read"], med["pft_read"] / med["edi_read"], lay.guaranteed_losses,
               med["pft_read_lossy"], med["pft_read_lossy"] / med["edi_read"], filled, E * sh.n_pf / 1e6))
        if not a.no_host and F == 16:
            edi_h = np.ascontiguousarray(sh.edi.cpu().numpy()[:, :n_af])
            t0 = time.perf_counter()
            pf_h = dabgpu.pft_fragments_host(lay, edi_h, sh.pseq)
            write_ms = 1e3 * (time.perf_counter() - t0)
            assert np.array_equal(pf_h, sh.pf.cpu().numpy()[:, :sh.n_pf]), "the host writer's fragments are not the device's"
            host = {}
            for name, src, n in (("whole", sh.pf, sh.n_pf), ("lossy", sh.lossy, sh.n_lossy)):
                data = src.cpu().numpy()
                out = np.empty((E, pad16(dabgpu.pft_read_out_bytes(n)) + 16), np.uint8)
                rec = np.empty((E, dabgpu.pft_read_max_records(n), 32), np.uint8)
                res, state = np.empty((E, 64), np.uint8), np.empty((E, dabgpu.pft_read_state_bytes() + 16), np.uint8)
                al = lambda x: x.ctypes.data + (-x.ctypes.data) % 16
                assert data.ctypes.data % 16 == 0 and data.strides[0] % 16 == 0
                entries = [dabgpu.PftReadEntry(data[k].ctypes.data, n, dabgpu.PFT_READ_FLUSH, None, al(state[k]), al(out[k]), rec[k].ctypes.data,
                                               res[k].ctypes.data) for k in range(E)]
                t0 = time.perf_counter()
                dabgpu.pft_read_host(entries)
                host[name] = 1e3 * (time.perf_counter() - t0)
                assert np.array_equal(res, sh.sides[name]["res"].cpu().numpy()), "the host reader's result is not the device's"
            row["F%d" % F].update(host_write_ms=write_ms, host_read_ms=host["whole"], host_read_lossy_ms=host["lossy"])
            print("     host calls, one thread, the same packets: writer %.1f ms (%.0f x the device call), reader %.1f ms (%.0f x), with the "
                  "missing fragments %.1f ms (%.0f x)" % (write_ms, write_ms / med["pft_write"], host["whole"], host["whole"] / med["pft_read"],
                                                          host["lossy"], host["lossy"] / med["pft_read_lossy"]))
    ctx.close()
    print(json.dumps(row))


if __name__ == "__main__":
    main()
