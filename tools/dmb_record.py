#!/usr/bin/env python3
"""ETI(NI) or EDI file -> one MPEG-2 transport stream file per T-DMB sub-channel.

  python tools/dmb_record.py in.eti out_prefix [--edi] [--chunk-bytes N] [--all-dscty]

The file (raw 6144-byte ETI(NI) frames, or with --edi AF packets back to back; both cut anywhere) is read on the device as
tools/eti_play.py and tools/edi_play.py read it: a discovery pass names the multiplex, then every call of --chunk-bytes bytes
goes through Context.eti_read / Context.edi_read.  The FIC says which sub-channels are stream-mode data
(dabgpu.fig_stream_components); those whose DSCTy is 24 (MPEG-2 transport stream; with --all-dscty every stream-mode data
sub-channel) go through Context.dmb_follow on the reader's rows, state handed on from call to call, and their 188-byte packets
are appended to out_prefix.<SubChId>.ts -- a file any TS tool opens.  The counters of every sub-channel, its PID census and
the programmes dabgpu.ts_programs finds in its first packets go to stderr.

An IQ recording is turned into ETI first: tools/eti_record.py capture.cf32 out.eti.  Uses nothing outside this repository."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dabgpu  # noqa: E402
from eti_play import groups_of_twelve  # noqa: E402


def discover(ctx, raw, dev, edi):
    """the multiplex the first good frame or packet of the file names -> [EtiStream]"""
    if edi:
        look = torch.from_numpy(raw[:min(raw.size, 1 << 18)].copy()).to(dev).reshape(1, -1)
        _f, _k, _o, status, result, _s = ctx.edi_read(look, None)
        status = status.cpu().numpy().view(dabgpu.EDI_READ_STATUS_DTYPE).reshape(-1)
        if not int(result.cpu().numpy().view(dabgpu.EDI_READ_RESULT_DTYPE).reshape(-1)[0]["rows"]):
            sys.exit("no DETI packet found in the first %d bytes" % look.numel())
        at, length = int(status[0]["offset"]), int(status[0]["length"])
        return dabgpu.edi_streams(raw[at:at + length])
    look = torch.from_numpy(raw[:min(raw.size, 64 * 6144)].copy()).to(dev).reshape(1, -1)
    _f, _k, _o, status, result, _s = ctx.eti_read(look, None)
    status = status.cpu().numpy().view(dabgpu.ETI_READ_STATUS_DTYPE).reshape(-1)
    found = int(result.cpu().numpy().view(dabgpu.ETI_READ_RESULT_DTYPE).reshape(-1)[0]["rows"])
    taken = [st for st in status[:found] if st["verdict"] == 0]
    if not taken:
        sys.exit("no ETI(NI) frame found in the first %d bytes" % look.numel())
    at = int(taken[0]["offset"])
    return dabgpu.eti_streams(raw[at:at + 6144])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input")
    ap.add_argument("out_prefix")
    ap.add_argument("--edi", action="store_true", help="the file holds AF packets, not ETI(NI) frames")
    ap.add_argument("--chunk-bytes", type=int, default=256 * 6144)
    ap.add_argument("--all-dscty", action="store_true", help="follow every stream-mode data sub-channel, whatever its DSCTy")
    a = ap.parse_args()
    raw = np.fromfile(a.input, np.uint8)
    dev = torch.device("cuda", 0)
    step = max(16, a.chunk_bytes // 16 * 16)
    with dabgpu.Context(device=0) as ctx:
        streams = discover(ctx, raw, dev, a.edi)
        read = ctx.edi_read if a.edi else ctx.eti_read
        result_dtype = dabgpu.EDI_READ_RESULT_DTYPE if a.edi else dabgpu.ETI_READ_RESULT_DTYPE
        by_start = {s.sc.start_address: k for k, s in enumerate(streams)}
        followed, state = None, None          # followed: [dict(comp, index, bitrate, state, file, totals, first)]
        for begin in range(0, raw.size, step):
            piece = torch.from_numpy(raw[begin:begin + step].copy()).to(dev).reshape(1, -1)
            fib, ok, outs, _status, result, state = read(piece, streams, state=state)
            rows = int(result.cpu().numpy().view(result_dtype).reshape(-1)[0]["rows"])
            if rows == 0:
                continue
            if followed is None:
                fib_h, ok_h = groups_of_twelve(fib[0, :rows].cpu().numpy(), ok[0, :rows].cpu().numpy())
                comps = [c for c in dabgpu.fig_stream_components(fib_h, ok_h)
                         if c.start_address in by_start and (a.all_dscty or c.dscty == dabgpu.DSCTY_MPEG2_TS)]
                if not comps:
                    continue                  # the FIC has not said yet what the streams are
                followed = []
                for c in comps:
                    k = by_start[c.start_address]
                    path = "%s.%d.ts" % (a.out_prefix, c.subchid)
                    followed.append(dict(comp=c, index=k, bitrate=streams[k].sc.bitrate_kbps, state=None, file=open(path, "wb"), path=path,
                                         totals=dict.fromkeys(dabgpu.DMB_COUNTERS, 0), last=None, first=[]))
            for f in followed:
                ts, _records, res, f["state"] = ctx.dmb_follow(outs[f["index"]][:, :rows], f["bitrate"], f["state"])
                res = res.cpu().numpy().view(dabgpu.DMB_RESULT_DTYPE).reshape(-1)[0]
                m = int(res["packets_emitted"])
                packets = ts[0, :m].cpu().numpy()
                f["file"].write(packets.tobytes())
                for k in dabgpu.DMB_COUNTERS:
                    f["totals"][k] += int(res[k])
                f["last"] = res
                if sum(len(p) for p in f["first"]) < 4096:
                    f["first"].append(packets)
        for f in followed or []:
            f["file"].close()
            c = f["comp"]
            print("sub-channel %d (SId 0x%X, DSCTy %d, %d kbit/s) -> %s" % (c.subchid, c.sid, c.dscty, f["bitrate"], f["path"]), file=sys.stderr)
            print("  " + " ".join("%s=%d" % kv for kv in f["totals"].items()), file=sys.stderr)
            if f["last"] is not None:
                print("  locked=%d phase=%d pids=%d pids_overflowed=%d" % tuple(int(f["last"][k]) for k in ("locked", "phase", "pids", "pids_overflowed")),
                      file=sys.stderr)
                for e in dabgpu.dmb_state_census(f["state"][0].cpu().numpy(), f["bitrate"]):
                    print("  pid 0x%04X: %d packets, %d discontinuities, %d duplicates, %d scrambled"
                          % (e["pid"], e["packets"], e["discontinuities"], e["duplicates"], e["scrambled"]), file=sys.stderr)
            if f["first"]:
                info = dabgpu.ts_programs(np.concatenate(f["first"]))
                for p in info.programs[:min(info.n_programs, dabgpu.TS_MAX_PROGRAMS)]:
                    es = ["0x%02X@0x%04X" % (p.stream_type[i], p.stream_pid[i]) for i in range(min(p.n_streams, dabgpu.TS_MAX_STREAMS))]
                    print("  programme %d: PMT 0x%04X%s" % (p.program_number, p.pmt_pid, (", PCR 0x%04X, IOD %s, streams %s" % (
                        p.pcr_pid, "yes" if p.iod_present else "no", " ".join(es))) if p.pmt_seen else " (not seen)"), file=sys.stderr)
        if not followed:
            print("no stream-mode data sub-channel%s announced" % ("" if a.all_dscty else " with DSCTy 24"), file=sys.stderr)


if __name__ == "__main__":
    main()
