#!/usr/bin/env python3
"""Time dabgpu_packet_groups_dev beside dabgpu_packet_slides_dev on the same frames: the packet-mode sub-channels of a batch of
ensembles (GPU box).

  python tools/packet_groups_time.py [--streams 64] [--frames 16,256] [--reps 20] [--out profiles/packet_groups_time.txt] [--limit 900]

One visit to the GPU, in a child process that is ended after --limit seconds.  The workload is that of
tools/packet_slides_time.py (same seeds): one or two packet-mode sub-channels of 32, 64 or 128 kbit/s per ensemble, each as
full of slide data as its 20-frame cycle has room for, in packets of four slots of one address.  The slides call assembles
those groups into MOT objects; the groups call gives every group with its header read and its CRC checked (keep_repeats 1:
nothing is held back), so it moves every group's bytes once, to d_bytes.  Per batch shape, after two warm-up calls of each,
--reps ROUNDS in one run, each round one slides call and one groups call timed between two events on the stream, by turns, so
that clock and neighbours are the same for both; reported: median, mean and least of the rounds.  Beside them the host twin
dabgpu_packet_groups_host on the same table in host memory (wall time, one thread), and the groups call on an address no
packet carries (the scan launch and a chunk loop with nothing to do)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from packet_slides_time import ADDRESS, NOBODY, cycle_frames                   # noqa: E402


def child(a):
    import numpy as np
    import torch
    import dabgpu
    from dabgpu import synth
    dev = torch.device("cuda", 0)
    prng = np.random.default_rng(2025)
    prates = [int(br) for _ in range(a.streams) for br in prng.choice([32, 64, 128], size=int(prng.integers(1, 3)))]
    lines = ["packet_groups_time: %d ensembles, %d packet sub-channels (%d kbit/s in all, %d..%d each) full of slide data, %s; the kernel takes "
             "%d followed packets at a time" % (a.streams, len(prates), sum(prates), min(prates), max(prates), torch.cuda.get_device_name(0),
                                                dabgpu.packet_groups_chunk())]
    cycle = {br: cycle_frames(synth, np, br)[0] for br in sorted(set(prates))}
    nb, gnb = dabgpu.packet_state_bytes(), dabgpu.packet_groups_state_bytes()
    cap, stride, slots = 8192, 8192 + 1024 + 256, 4
    ab = dabgpu.mot_arena_bytes(cap)

    def stats(ms):
        ms = sorted(ms)
        return "median %8.3f  mean %8.3f  least %8.3f ms" % (ms[len(ms) // 2], sum(ms) / len(ms), ms[0])

    with dabgpu.Context(device=0, max_frames=64) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)

        def event_ms(run):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run()
            e1.record(stream)
            ctx.sync()
            return e0.elapsed_time(e1)

        for fps in a.frames:
            n_cifs = 4 * fps
            keep, pswap, gswap, nobody, hswap, gcnts = [], [[], []], [[], []], [], [[], []], []
            for e, br in enumerate(prates):
                host = np.ascontiguousarray(cycle[br][(np.arange(n_cifs) - e % 7) % 20])
                frames = torch.from_numpy(host).to(dev)
                s0, s1 = (torch.zeros((nb,), dtype=torch.uint8, device=dev) for _ in range(2))
                g0, g1 = (torch.zeros((gnb,), dtype=torch.uint8, device=dev) for _ in range(2))
                arena = torch.zeros((ab,), dtype=torch.uint8, device=dev)
                slides = torch.zeros((slots, stride), dtype=torch.uint8, device=dev)
                cnt = torch.zeros((192,), dtype=torch.uint8, device=dev)
                # every useful byte of the call has room: 3 R bytes a frame, and 15 bytes of rounding for each of at most n_cifs S groups
                max_groups = n_cifs * br // 8
                capacity = n_cifs * 3 * br + 16 * max_groups
                out = torch.zeros((capacity,), dtype=torch.uint8, device=dev)
                recs = torch.zeros((max_groups * 32,), dtype=torch.uint8, device=dev)
                gcnt = torch.zeros((112,), dtype=torch.uint8, device=dev)
                h = [np.zeros(gnb + 16, np.uint8), np.zeros(gnb + 16, np.uint8), np.zeros(capacity + 16, np.uint8), np.zeros(max_groups * 32 + 16, np.uint8),
                     np.zeros(112, np.uint8)]
                al = [x[-x.ctypes.data % 16:] for x in h[:4]]
                keep += [frames, s0, s1, g0, g1, arena, slides, cnt, out, recs, host, h]
                gcnts.append(gcnt)
                for side, (si, so, gi, go) in enumerate(((s0, s1, g0, g1), (s1, s0, g1, g0))):
                    pswap[side].append(dabgpu.PacketEntry(frames.data_ptr(), 3 * br, br, ADDRESS, 0, 0, si.data_ptr(), so.data_ptr(), arena.data_ptr(), ab,
                                                          slides.data_ptr(), stride, slots, 0, cnt.data_ptr()))
                    gswap[side].append(dabgpu.PacketGroupsEntry(frames.data_ptr(), 3 * br, br, ADDRESS, 0, 0, 1, 0, gi.data_ptr(), go.data_ptr(), out.data_ptr(),
                                                                recs.data_ptr(), capacity, max_groups, gcnt.data_ptr()))
                    hswap[side].append(dabgpu.PacketGroupsEntry(host.ctypes.data, 3 * br, br, ADDRESS, 0, 0, 1, 0, al[side].ctypes.data, al[side ^ 1].ctypes.data,
                                                                al[2].ctypes.data, al[3].ctypes.data, capacity, max_groups, h[4].ctypes.data))
                nobody.append(dabgpu.PacketGroupsEntry(frames.data_ptr(), 3 * br, br, NOBODY, 0, 0, 1, 0, None, g0.data_ptr(), out.data_ptr(), recs.data_ptr(),
                                                       capacity, max_groups, gcnt.data_ptr()))
            torch.cuda.synchronize()
            turn = [0, 0, 0]

            def slides_call():
                ctx.packet_slides_dev(pswap[turn[0]], n_cifs)
                turn[0] ^= 1

            def groups_call():
                ctx.packet_groups_dev(gswap[turn[1]], n_cifs)
                turn[1] ^= 1

            for _ in range(2):
                slides_call()
                groups_call()
            ctx.sync()
            ms_slides, ms_groups = [], []
            for _ in range(a.reps):
                ms_slides.append(event_ms(slides_call))
                ms_groups.append(event_ms(groups_call))
            gc = np.stack([c.cpu().numpy().view(dabgpu.PACKET_GROUPS_RESULT_DTYPE)[0] for c in gcnts])
            ms_nobody = [event_ms(lambda: ctx.packet_groups_dev(nobody, n_cifs)) for _ in range(a.reps)]
            t0 = time.perf_counter()
            for _ in range(max(1, a.reps // 4)):
                dabgpu.packet_groups_host(hswap[turn[2]], n_cifs)
                turn[2] ^= 1
            wall_host = (time.perf_counter() - t0) * 1e3 / max(1, a.reps // 4)
            med = lambda v: sorted(v)[len(v) // 2]                    # noqa: E731
            lines += ["%d x %d frames (%d logical frames per entry; the last groups call scanned %d slots: %d followed packets, %d groups closed, %d emitted, "
                      "%d without room, %d CRC failed, %d bytes emitted):" %
                      (a.streams, fps, n_cifs, gc["slots"].sum(), gc["packets_followed"].sum(), gc["groups_closed"].sum(), gc["groups_emitted"].sum(),
                       gc["groups_no_room"].sum(), gc["groups_crc_failed"].sum(), gc["bytes_emitted"].sum()),
                      "  dabgpu_packet_slides_dev, between events   %s  (%d rounds, by turns with the next line)" % (stats(ms_slides), a.reps),
                      "  dabgpu_packet_groups_dev, between events   %s  groups / slides = %.3f by the medians" % (stats(ms_groups), med(ms_groups) / med(ms_slides)),
                      "  the groups call, nothing to follow         %s  (the scan launch and an idle chunk loop)" % stats(ms_nobody),
                      "  dabgpu_packet_groups_host, same table      %8.3f ms wall, one thread" % wall_host]
            del keep, pswap, gswap, nobody, hswap, gcnts
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", default="16,256", help="frames per stream, one batch shape each")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packet_groups_time.txt"))
    ap.add_argument("--limit", type=int, default=900, help="seconds the GPU visit may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        a.frames = [int(x) for x in a.frames.split(",")]
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--streams", str(a.streams), "--frames", a.frames, "--reps", str(a.reps),
           "--out", a.out]
    try:
        sys.exit(subprocess.run(cmd, timeout=a.limit).returncode)
    except subprocess.TimeoutExpired:
        sys.exit("packet_groups_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
