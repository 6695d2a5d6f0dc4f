#!/usr/bin/env python3
"""ETI(NI) file -> what is in it: ensemble, services, dynamic labels, slides, and the reader's counters.

  python tools/eti_play.py file.eti [--chunk-frames N]

The file holds raw 6144-byte ETI(NI) frames one after the other; it may begin and end anywhere and bytes may be missing in
the middle (the reader resynchronises).  The length-prefixed framings other tools write around ETI frames are NOT read:
strip them first.  A discovery pass (Context.eti_read without a plan) finds the first good frame, its STC gives the
multiplex (eti_streams), then the file is read in calls of --chunk-frames frames with the unfinished tail carried from call
to call, and every DAB+, layer-II and packet-mode MOT component is followed with the calls that follow them behind the
channel decoder (dabplus_follow_dev / mp2_follow_dev -> pad_labels_dev + mot_slides_dev, packet_slides_dev).  A call that
lost bytes emits fewer rows; every call follows the rows it got.  Uses nothing outside this repository."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dabgpu  # noqa: E402
from oracle import fig_oracle as FO  # noqa: E402

BODY_CAPACITY, MAX_SLIDES = 64 * 1024, 8
SLOT = 32 + 1024 + BODY_CAPACITY


def groups_of_twelve(fib, ok):
    """[rows][3][32] / [rows][3] as the FIG functions take them: [n][12][32] / [n][12] (FIBs without a row: CRC flag 0)"""
    rows = fib.shape[0]
    n = (rows + 3) // 4
    f, k = np.zeros((n * 4, 3, 32), np.uint8), np.zeros((n * 4, 3), np.uint8)
    f[:rows], k[:rows] = fib, ok
    return f.reshape(n, 12, 32), k.reshape(n, 12)


class Followed:
    """One followed component: its buffers on the device, swapped from call to call."""

    def __init__(self, kind, index, bitrate, comp, dev):
        z = lambda n: torch.zeros(max(int(n), 1), dtype=torch.uint8, device=dev)
        self.kind, self.index, self.bitrate, self.comp, self.calls = kind, index, bitrate, comp, 0
        carry = {"dab+": dabgpu.dabplus_carry_bytes, "dab": dabgpu.mp2_carry_bytes}.get(kind, lambda b: 0)(bitrate)
        self.carry = [z(carry), z(carry)]
        self.pad = [z(dabgpu.pad_state_bytes()), z(dabgpu.pad_state_bytes())]
        state = dabgpu.packet_state_bytes() if kind == "packet" else dabgpu.mot_state_bytes()
        self.mot = [z(state), z(state)]
        self.arena = z(dabgpu.mot_arena_bytes(BODY_CAPACITY))
        self.label = z(144)
        self.slides, self.frames, self.units = [], 0, 0

    def swap(self):
        for pair in (self.carry, self.pad, self.mot):
            pair.reverse()
        self.calls += 1


def play(ctx, raw, dev, streams, read, step, result_dtype):
    """The file's bytes through `read` (Context.eti_read or Context.edi_read: the same arguments, the same returns) in calls
    of `step` bytes, every component followed, and what was found printed.  -> the read counters (a record of result_dtype)"""
    by_start = {s.sc.start_address: k for k, s in enumerate(streams)}
    followed, fibs_seen, totals, state = None, [], np.zeros(1, result_dtype), None
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)
    for begin in range(0, raw.size, step):
        piece = torch.from_numpy(raw[begin:begin + step].copy()).to(dev).reshape(1, -1)
        fib, ok, outs, _status, result, state = read(piece, streams, state=state)
        res = result.cpu().numpy().view(result_dtype).reshape(-1)[0]
        for k in totals.dtype.names[:8]:
            totals[k] += res[k]
        totals["tail_bytes"] = res["tail_bytes"]
        rows = int(res["rows"])
        if rows == 0:
            continue
        fib_h, ok_h = groups_of_twelve(fib[0, :rows].cpu().numpy(), ok[0, :rows].cpu().numpy())
        fibs_seen.append(fib_h.reshape(-1, 32)[ok_h.reshape(-1) != 0])
        if followed is None:
            audio = [c for c in dabgpu.fig_audio_components(fib_h, ok_h) if c.start_address in by_start]
            packets = [c for c in dabgpu.fig_packet_components(fib_h, ok_h)
                       if c.start_address in by_start and c.dscty == dabgpu.DSCTY_MOT and c.dg_flag == 0]
            if not audio and not packets:
                continue                                  # the FIC has not said yet what the streams are
            followed = [Followed("dab+" if c.ascty == dabgpu.ASCTY_DABPLUS else "dab", by_start[c.start_address],
                                 streams[by_start[c.start_address]].sc.bitrate_kbps, c, dev) for c in audio]
            followed += [Followed("packet", by_start[c.start_address], streams[by_start[c.start_address]].sc.bitrate_kbps, c, dev)
                         for c in packets]
        # the follow calls of this call's rows, all behind one another on the context's stream
        max_sf, keep = (rows + 4) // 5, []
        sources = {}
        for f in followed:
            d_in, nb = outs[f.index][0], 3 * f.bitrate
            first = None if f.calls == 0 else f.carry[0].data_ptr()
            if f.kind == "dab+":
                data, st, res_f = z(max_sf, 110 * f.bitrate // 8), z(max_sf * 64), z(32)
                ctx.dabplus_follow_dev([dabgpu.DabplusEntry(d_in.data_ptr(), nb, f.bitrate, first, f.carry[1].data_ptr(), data.data_ptr(),
                                                            st.data_ptr(), res_f.data_ptr())], rows)
                sources[id(f)] = (data.data_ptr(), 110 * f.bitrate // 8, st.data_ptr(), res_f.data_ptr(), f.bitrate, max_sf)
                keep += [data, st, res_f]
                f.result = res_f
            elif f.kind == "dab":
                data, st, res_f, res_m = z(rows + 1, dabgpu.MP2_ROW_BYTES), z((rows + 1) * 64), z(32), z(64)
                ctx.mp2_follow_dev([dabgpu.Mp2Entry(d_in.data_ptr(), nb, f.bitrate, first, f.carry[1].data_ptr(), data.data_ptr(), st.data_ptr(),
                                                    res_f.data_ptr(), res_m.data_ptr())], rows)
                sources[id(f)] = (data.data_ptr(), dabgpu.MP2_ROW_BYTES, st.data_ptr(), res_f.data_ptr(), dabgpu.MP2_PAD_KBPS, rows + 1)
                keep += [data, st, res_f, res_m]
                f.result = res_m
            f.slots, f.mot_result = torch.zeros((MAX_SLIDES, SLOT), dtype=torch.uint8, device=dev), z(192)
            mot_in = None if f.calls == 0 else f.mot[0].data_ptr()
            if f.kind == "packet":
                ctx.packet_slides_dev([dabgpu.PacketEntry(d_in.data_ptr(), nb, f.bitrate, f.comp.packet_address, f.comp.fec_scheme, 0, mot_in,
                                                          f.mot[1].data_ptr(), f.arena.data_ptr(), f.arena.numel(), f.slots.data_ptr(), SLOT,
                                                          MAX_SLIDES, 0, f.mot_result.data_ptr())], rows)
                continue
            pad_result = z(64)
            keep.append(pad_result)
            ctx.mot_slides_dev([dabgpu.MotEntry(*sources[id(f)], mot_in, f.mot[1].data_ptr(), f.arena.data_ptr(), f.arena.numel(),
                                                f.slots.data_ptr(), SLOT, MAX_SLIDES, 0, f.mot_result.data_ptr())])
            ctx.pad_labels_dev([dabgpu.PadEntry(*sources[id(f)], None if f.calls == 0 else f.pad[0].data_ptr(), f.pad[1].data_ptr(),
                                                f.label.data_ptr(), pad_result.data_ptr())])
        ctx.sync()
        for f in followed:
            if f.kind == "packet":
                mot = f.mot_result.cpu().numpy().view(dabgpu.PACKET_RESULT_DTYPE)[0]
                f.frames += int(mot["cifs"])
                mot = mot["mot"]
            else:
                mot = f.mot_result[:128].cpu().numpy().view(dabgpu.MOT_RESULT_DTYPE)[0]
                if f.kind == "dab+":
                    f.units += int(f.result.cpu().numpy().view(dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)["n_superframes"][0])
                else:
                    f.frames += int(f.result.cpu().numpy().view(dabgpu.MP2_RESULT_DTYPE)["frames"][0])
            slots = f.slots.cpu().numpy()
            for k in range(min(int(mot["slides_written"]), MAX_SLIDES)):
                rec = slots[k, :32].copy().view(dabgpu.MOT_SLIDE_DTYPE)[0]
                header = slots[k, 32:32 + int(rec["header_bytes"])].tobytes()
                f.slides.append((int(rec["transport_id"]), dabgpu.mot_header_parse(header).get("name", b""), int(rec["body_bytes"])))
            f.swap()
    # what the FIC says: ensemble and services with their labels
    if fibs_seen:
        for line in FO.parse_fibs(np.concatenate(fibs_seen)).lines():
            if line.split()[0] in ("ensemble", "service", "subchannel", "component"):
                print(line)
    for f in followed or []:
        s = streams[f.index]
        what = {"dab+": "%d super-frames" % f.units, "dab": "%d layer-II frames" % f.frames, "packet": "%d frames, packet address %d" %
                (f.frames, f.comp.packet_address if f.kind == "packet" else 0)}[f.kind]
        line = "followed %s sid=0x%X subchannel=%d start=%d %d kbit/s: %s" % (f.kind, f.comp.sid, s.subchannel_id, s.sc.start_address, f.bitrate, what)
        if f.kind != "packet":
            lab = f.label.cpu().numpy().view(dabgpu.PAD_LABEL_DTYPE)[0]
            try:
                text = dabgpu.pad_label_utf8(lab) if int(lab["length"]) else ""
            except dabgpu.DabGpuError:
                text = lab["text"][:int(lab["length"])].tobytes().decode("latin-1")
            line += ", label %r" % text
        print(line)
        for tid, name, size in f.slides:
            print("  slide transport_id=0x%X name=%r %d bytes" % (tid, name, size))
    return totals[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("eti", help="raw 6144-byte ETI(NI) frames, cut anywhere (no length-prefixed framing)")
    ap.add_argument("--chunk-frames", type=int, default=256, help="frames' worth of bytes per read call")
    a = ap.parse_args()
    raw = np.fromfile(a.eti, np.uint8)
    dev = torch.device("cuda", 0)
    with dabgpu.Context(device=0) as ctx:
        # discovery: the first good frame of the file names the multiplex
        look = torch.from_numpy(raw[:min(raw.size, 64 * 6144)].copy()).to(dev).reshape(1, -1)
        _f, _k, _o, status, result, _s = ctx.eti_read(look, None)
        status = status.cpu().numpy().view(dabgpu.ETI_READ_STATUS_DTYPE).reshape(-1)
        found = int(result.cpu().numpy().view(dabgpu.ETI_READ_RESULT_DTYPE).reshape(-1)[0]["rows"])
        taken = [st for st in status[:found] if st["verdict"] == 0]
        if not taken:
            sys.exit("no ETI(NI) frame found in the first %d bytes of %s" % (look.numel(), a.eti))
        at = int(taken[0]["offset"])
        streams = dabgpu.eti_streams(raw[at:at + 6144])
        print("multiplex of the frame at byte %d: %d streams %s" % (at, len(streams), [(s.subchannel_id, s.sc.start_address, s.sc.bitrate_kbps) for s in streams]))
        t = play(ctx, raw, dev, streams, ctx.eti_read, a.chunk_frames * 6144, dabgpu.ETI_READ_RESULT_DTYPE)
        print("read: " + " ".join("%s=%d" % (k, int(t[k])) for k in t.dtype.names[:9]))


if __name__ == "__main__":
    main()
