#!/usr/bin/env python3
"""Time dabgpu_packet_slides_dev on the packet-mode sub-channels of a batch of ensembles, beside dabgpu_dabplus_follow_dev on
the DAB+ entries of the same batch and against the host twin on the same table (GPU box).

  python tools/packet_slides_time.py [--streams 64] [--frames 16,256] [--reps 20] [--out profiles/packet_slides_time.txt] [--limit 900]

One visit to the GPU, in a child process that is ended after --limit seconds.  The workload is the monitoring shape of
tools/pad_slides_time.py (same plans, same seed) with one or two packet-mode sub-channels of 32, 64 or 128 kbit/s added to
every ensemble, each as full of slide data as its 20-frame cycle has room for: two slideshow objects (two transport ids, so
that each of them completes in every cycle) in packets of four slots of one address.  Per batch shape the child times, over
--reps repetitions after two warm-up calls, as stream-synchronised wall time and between two events on the stream:
  (a) the DAB+ follow call alone, the carry records swapped between calls
  (b) the packet call with an address no packet carries: the scan launch, and a walk launch that only sums the scan's records
  (c) the packet call on the address that carries the slides, the state records swapped, the arena in place: both launches at work;
      (c) - (b) is what the walk launch spends on the followed packets
  (d) (a) and (c) in sequence on the same stream
  (e) the host twin dabgpu_packet_slides_host on the same table in host memory (wall time, one thread)
and a plain device-to-device copy of as many bytes as the packet call moved."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

ADDRESS, NOBODY = 7, 8


def cycle_frames(synth, np, br):
    """20 logical frames of a packet sub-channel at this bit rate, as full of two slides as they get -> (frames, body bytes)"""
    body = 20 * (br // 8) * 24 * 9 // 10
    while True:
        groups = []
        for k in range(2):
            data = bytes(np.random.default_rng(br * 2 + k).integers(0, 256, body // 2, dtype=np.uint8))
            groups += synth.mot_object_groups(0x4000 + 2 * br + k, synth.slide_header(len(data), b"slide-%d-%d.jpg" % (br, k)), data, 1024)
        packets = synth.packetise(groups, ADDRESS, sizes=(4,))
        while len(packets) % 4:
            packets.append(synth.packet(ADDRESS, b"\x00", 1, ci=len(packets), command=True))
        frames = synth.packet_frames(br, [packets], n_frames=20)
        if len(frames) == 20:
            return frames, body
        body = body * 19 // 20


def child(a):
    import numpy as np
    import torch
    import dabgpu
    from dabgpu import synth
    from ensembles_time import random_plan
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2024)
    plans = [random_plan(dabgpu, rng) for _ in range(a.streams)]
    rates = [sc.bitrate_kbps for p in plans for sc in p if not sc.is_uep]
    prng = np.random.default_rng(2025)
    prates = [int(br) for _ in range(a.streams) for br in prng.choice([32, 64, 128], size=int(prng.integers(1, 3)))]
    lines = ["packet_slides_time: %d ensembles, %d packet sub-channels (%d kbit/s in all, %d..%d each) full of slide data, beside %d DAB+ entries "
             "(%d kbit/s in all), %s" % (a.streams, len(prates), sum(prates), min(prates), max(prates), len(rates), sum(rates),
                                         torch.cuda.get_device_name(0))]
    cycle, carried = {}, {}
    for br in sorted(set(prates)):
        cycle[br], carried[br] = cycle_frames(synth, np, br)
    lines.append("slide bytes per cycle of 20 logical frames, by bit rate: " + ", ".join("%d: %d" % (br, carried[br]) for br in sorted(carried)))
    audio = {br: np.concatenate([synth.build_superframe(rng, br, 1, 1)[0] for _q in range(4)]).reshape(20, 3 * br) for br in sorted(set(rates))}
    nb, cap, stride, slots = dabgpu.packet_state_bytes(), 8192, 8192 + 1024 + 256, 4
    ab = dabgpu.mot_arena_bytes(cap)

    with dabgpu.Context(device=0, max_frames=64) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)

        def timed(run):
            for _ in range(2):
                run()
            ctx.sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            for _ in range(a.reps):
                run()
            e1.record(stream)
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3 / a.reps, e0.elapsed_time(e1) / a.reps

        for fps in a.frames:
            n_cifs, max_sf = 4 * fps, (4 * fps + 4) // 5
            keep, swap, pswap, nobody, hswap, cnts, states = [], [[], []], [[], []], [], [[], []], [], []
            for e, br in enumerate(rates):
                frames = torch.from_numpy(np.ascontiguousarray(audio[br][(np.arange(n_cifs) - e % 5) % 20])).to(dev)
                data = torch.zeros((max_sf, 110 * br // 8), dtype=torch.uint8, device=dev)
                st = torch.zeros((max_sf * 64,), dtype=torch.uint8, device=dev)
                res = torch.zeros((32,), dtype=torch.uint8, device=dev)
                c0, c1 = (torch.zeros((dabgpu.dabplus_carry_bytes(br),), dtype=torch.uint8, device=dev) for _ in range(2))
                keep += [frames, data, st, res, c0, c1]
                for side, (ci, co) in enumerate(((c0, c1), (c1, c0))):
                    swap[side].append(dabgpu.DabplusEntry(frames.data_ptr(), 3 * br, br, ci.data_ptr(), co.data_ptr(), data.data_ptr(), st.data_ptr(), res.data_ptr()))
            for e, br in enumerate(prates):
                host = np.ascontiguousarray(cycle[br][(np.arange(n_cifs) - e % 7) % 20])
                frames = torch.from_numpy(host).to(dev)
                s0, s1 = (torch.zeros((nb,), dtype=torch.uint8, device=dev) for _ in range(2))
                arena = torch.zeros((ab,), dtype=torch.uint8, device=dev)
                slides = torch.zeros((slots, stride), dtype=torch.uint8, device=dev)
                cnt = torch.zeros((192,), dtype=torch.uint8, device=dev)
                h = [np.zeros(nb + 16, np.uint8), np.zeros(nb + 16, np.uint8), np.zeros(ab + 16, np.uint8), np.zeros(slots * stride + 16, np.uint8), np.zeros(192, np.uint8)]
                al = [x[-x.ctypes.data % 16:] for x in h[:4]]
                keep += [frames, arena, slides, host, h]
                states += [s0, s1]
                cnts.append(cnt)
                for side, (si, so) in enumerate(((s0, s1), (s1, s0))):
                    pswap[side].append(dabgpu.PacketEntry(frames.data_ptr(), 3 * br, br, ADDRESS, 0, 0, si.data_ptr(), so.data_ptr(), arena.data_ptr(), ab,
                                                          slides.data_ptr(), stride, slots, 0, cnt.data_ptr()))
                    hswap[side].append(dabgpu.PacketEntry(host.ctypes.data, 3 * br, br, ADDRESS, 0, 0, al[side].ctypes.data, al[side ^ 1].ctypes.data,
                                                          al[2].ctypes.data, ab, al[3].ctypes.data, stride, slots, 0, h[4].ctypes.data))
                nobody.append(dabgpu.PacketEntry(frames.data_ptr(), 3 * br, br, NOBODY, 0, 0, None, s0.data_ptr(), arena.data_ptr(), ab, slides.data_ptr(),
                                                 stride, slots, 0, cnt.data_ptr()))
            torch.cuda.synchronize()
            turn = [0, 0, 0]

            def follow():
                ctx.dabplus_follow_dev(swap[turn[0]], n_cifs)
                turn[0] ^= 1

            def packets():
                ctx.packet_slides_dev(pswap[turn[1]], n_cifs)
                turn[1] ^= 1

            def both():
                follow()
                packets()

            wall_a, dev_a = timed(follow)
            wall_b, dev_b = timed(lambda: ctx.packet_slides_dev(nobody, n_cifs))
            for s in states:                                          # (the run above left its state in the first record)
                s.zero_()
            wall_c, dev_c = timed(packets)
            wall_d, dev_d = timed(both)
            pc = np.stack([c.cpu().numpy().view(dabgpu.PACKET_RESULT_DTYPE)[0] for c in cnts])
            t0 = time.perf_counter()
            for _ in range(a.reps):
                dabgpu.packet_slides_host(hswap[turn[2]], n_cifs)
                turn[2] ^= 1
            wall_e = (time.perf_counter() - t0) * 1e3 / a.reps
            moved = int(pc["group_bytes"].sum()) + int(pc["mot"]["object_bytes"].sum())
            src, dst = (torch.zeros((max(moved, 16),), dtype=torch.uint8, device=dev) for _ in range(2))
            with torch.cuda.stream(stream):
                wall_f, dev_f = timed(lambda: dst.copy_(src))
            lines += ["%d x %d frames (%d logical frames per entry; the last packet call scanned %d slots: %d bad, %d padding packets, %d followed; %d "
                      "continuity breaks; %d groups ok, %d CRC failed; %d segments placed, %d objects completed, %d slides written, %d dropped; %d "
                      "bytes into data groups, %d bytes into objects and slots):" %
                      (a.streams, fps, n_cifs, pc["slots"].sum(), pc["slots_bad"].sum(), pc["packets_padding"].sum(), pc["packets_followed"].sum(),
                       pc["continuity_breaks"].sum(), pc["mot"]["groups_ok"].sum(), pc["mot"]["groups_crc_failed"].sum(), pc["mot"]["segments_placed"].sum(),
                       pc["mot"]["objects_completed"].sum(), pc["mot"]["slides_written"].sum(), pc["mot"]["slides_dropped"].sum(), pc["group_bytes"].sum(),
                       pc["mot"]["object_bytes"].sum()),
                      "  (a) the DAB+ follow call alone          %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_a, dev_a, a.reps),
                      "  (b) scan + a walk with nothing to follow %8.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_b, dev_b, a.reps),
                      "  (c) the packet call, slides followed    %9.3f ms wall  %9.3f ms between events  (mean of %d)   (c) - (b) = %.3f ms between events: the walk's packets"
                      % (wall_c, dev_c, a.reps, dev_c - dev_b),
                      "  (d) (a) then (c) on the same stream     %9.3f ms wall  %9.3f ms between events  (mean of %d)   (d) / (a) = %.2f wall, %.2f events"
                      % (wall_d, dev_d, a.reps, wall_d / wall_a, dev_d / dev_a),
                      "  (e) the host twin on the same table     %9.3f ms wall, one thread                               (e) / (c) = %.1f wall" % (wall_e, wall_e / wall_c),
                      "      a plain device copy of the %d bytes moved: %.3f ms wall  %.3f ms between events" % (moved, wall_f, dev_f)]
            del keep, swap, pswap, nobody, hswap, cnts, states
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packet_slides_time.txt"))
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
        sys.exit("packet_slides_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
