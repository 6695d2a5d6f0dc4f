#!/usr/bin/env python3
"""EDI file -> what is in it: ensemble, services, dynamic labels, slides, and the reader's counters.

  python tools/edi_play.py file.edi [--chunk-bytes N] [--host] [--pft]

The file is an AF packet stream, as a capture of a multiplexer's TCP output is: packets back to back; it may begin and end
anywhere, bytes may be missing in the middle and packets that are no DETI packets may lie between (the reader steps over
them and resynchronises).  With --pft the file is a PF fragment stream instead (datagram payloads one after the other, as
tools/edi_record.py --pft writes them): the PFT reader (Context.pft_read, or pft_read_host with --host) puts the AF packets
back together first, fragments in any order, missing ones filled by RS(255,207) where they can be, and its counters are
listed.  UDP datagram framings (pcap and the like) are NOT read.  A discovery pass (Context.edi_read without a
plan) finds the first DETI packet, its est items give the multiplex (edi_streams), then the file is read in calls of
--chunk-bytes bytes with the unfinished tail carried from call to call and every DAB+, layer-II and packet-mode MOT component is
followed exactly as tools/eti_play.py follows them (its play()).  --host reads with edi_read_host instead and needs no GPU: the
multiplex, what the FIC says (ensemble, services, sub-channels, components) and the reader's counters are listed, the
components are not followed (labels and slides come from the follow calls, which run on the device).  Uses nothing outside
this repository."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import dabgpu  # noqa: E402
from oracle import fig_oracle as FO  # noqa: E402


def aligned(n):
    raw = np.zeros(n + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n]


def read_host(data, plan, state):
    """one call of edi_read_host on one stream -> (fib [rows][96], crc_ok [rows][3], status [rows], result record, state)"""
    rows = dabgpu.edi_read_max_rows(data.size, plan)
    buf = aligned(max(data.size, 1))
    buf[:data.size] = data
    fib, ok, status, result = aligned(rows * 96), aligned(rows * 3), aligned(rows * 32), aligned(48)
    state_out = aligned(dabgpu.edi_read_state_bytes())
    dabgpu.edi_read_host([dabgpu.EdiReadEntry(buf.ctypes.data if data.size else None, data.size, 0, None if plan is None else C.pointer(plan),
                                              None, None if state is None else state.ctypes.data, state_out.ctypes.data, fib.ctypes.data,
                                              ok.ctypes.data, status.ctypes.data, result.ctypes.data)])
    res = result.view(dabgpu.EDI_READ_RESULT_DTYPE)[0]
    n = int(res["rows"])
    return fib.reshape(-1, 96)[:n], ok.reshape(-1, 3)[:n], status.view(dabgpu.EDI_READ_STATUS_DTYPE)[:n], res, state_out


def describe(at, st, streams):
    print("multiplex of the packet at byte %d (dlfc %d, SEQ %d): %d streams %s"
          % (at, int(st["dlfc"]), int(st["seq"]), len(streams), [(s.subchannel_id, s.sc.start_address, s.sc.bitrate_kbps) for s in streams]))


def pft_to_af(raw, chunk, ctx=None):
    """a PF fragment stream -> its AF packets back to back, read in calls of `chunk` bytes with the state carried"""
    pieces, state, totals = [], None, np.zeros(1, dabgpu.PFT_READ_RESULT_DTYPE)
    begins = list(range(0, raw.size, chunk)) or [0]
    for begin in begins:
        data, last = raw[begin:begin + chunk], begin == begins[-1]
        if ctx is None:
            buf, out = aligned(max(data.size, 1)), aligned(dabgpu.pft_read_out_bytes(data.size))
            buf[:data.size] = data
            rec, res, state_out = aligned(dabgpu.pft_read_max_records(data.size) * 32), aligned(64), aligned(dabgpu.pft_read_state_bytes())
            dabgpu.pft_read_host([dabgpu.PftReadEntry(buf.ctypes.data if data.size else None, data.size, dabgpu.PFT_READ_FLUSH if last else 0,
                                                      None if state is None else state.ctypes.data, state_out.ctypes.data, out.ctypes.data,
                                                      rec.ctypes.data, res.ctypes.data)])
            res, state = res.view(dabgpu.PFT_READ_RESULT_DTYPE)[0], state_out
        else:
            import torch
            out, _rec, res, state = ctx.pft_read(torch.from_numpy(data.copy()).cuda().reshape(1, -1), state, flush=last)
            res, out = res.cpu().numpy().view(dabgpu.PFT_READ_RESULT_DTYPE).reshape(-1)[0], out[0, :].cpu().numpy()
        pieces.append(out[:int(res["out_bytes"])].copy())
        for k in totals.dtype.names:
            totals[k] += res[k]
        totals["tail_bytes"] = res["tail_bytes"]
    print("pft: " + " ".join("%s=%d" % (k, int(totals[0][k])) for k in totals.dtype.names))
    return np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)


def main_host(raw, chunk):
    _f, _k, status, _r, _s = read_host(raw[:min(raw.size, 1 << 18)], None, None)
    if not len(status):
        sys.exit("no DETI packet found in the first %d bytes" % min(raw.size, 1 << 18))
    at, length = int(status[0]["offset"]), int(status[0]["length"])
    streams = dabgpu.edi_streams(raw[at:at + length])
    describe(at, status[0], streams)
    plan = dabgpu.eti_layout(streams)
    totals, state, good = np.zeros(1, dabgpu.EDI_READ_RESULT_DTYPE), None, []
    for begin in range(0, raw.size, chunk):
        fib, ok, _status, res, state = read_host(raw[begin:begin + chunk], plan, state)
        for k in totals.dtype.names[:8]:
            totals[k] += res[k]
        totals["tail_bytes"] = res["tail_bytes"]
        good.append(fib.reshape(-1, 32)[ok.reshape(-1) != 0])
    if good:
        for line in FO.parse_fibs(np.concatenate(good)).lines():
            if line.split()[0] in ("ensemble", "service", "subchannel", "component"):
                print(line)
    print("read: " + " ".join("%s=%d" % (k, int(totals[0][k])) for k in totals.dtype.names[:9]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("edi", help="AF packets back to back, cut anywhere (no PFT, no datagram framing)")
    ap.add_argument("--chunk-bytes", type=int, default=1 << 20, help="bytes per read call")
    ap.add_argument("--host", action="store_true", help="read on the host (no GPU): the FIC's listing and the counters only")
    ap.add_argument("--pft", action="store_true", help="the file holds PF fragments (EDI as it travels over UDP), not AF packets")
    a = ap.parse_args()
    raw = np.fromfile(a.edi, np.uint8)
    if a.host:
        return main_host(pft_to_af(raw, a.chunk_bytes) if a.pft else raw, a.chunk_bytes)
    import torch
    from eti_play import play
    dev = torch.device("cuda", 0)
    with dabgpu.Context(device=0) as ctx:
        if a.pft:
            raw = pft_to_af(raw, a.chunk_bytes, ctx)
        # discovery: the first DETI packet of the file names the multiplex
        look = torch.from_numpy(raw[:min(raw.size, 1 << 18)].copy()).to(dev).reshape(1, -1)
        _f, _k, _o, status, result, _s = ctx.edi_read(look, None)
        status = status.cpu().numpy().view(dabgpu.EDI_READ_STATUS_DTYPE).reshape(-1)
        found = int(result.cpu().numpy().view(dabgpu.EDI_READ_RESULT_DTYPE).reshape(-1)[0]["rows"])
        if not found:
            sys.exit("no DETI packet found in the first %d bytes of %s" % (look.numel(), a.edi))
        at, length = int(status[0]["offset"]), int(status[0]["length"])
        streams = dabgpu.edi_streams(raw[at:at + length])
        describe(at, status[0], streams)
        t = play(ctx, raw, dev, streams, ctx.edi_read, a.chunk_bytes, dabgpu.EDI_READ_RESULT_DTYPE)
        print("read: " + " ".join("%s=%d" % (k, int(t[k])) for k in t.dtype.names[:9]))


if __name__ == "__main__":
    main()
