#!/usr/bin/env python3
"""Time dabgpu_packet_fec_dev on the packet-mode sub-channels of tools/packet_slides_time.py's batch (same seed: 64 ensembles,
94 packet sub-channels of 32, 64 or 128 kbit/s), now with FEC frames, against the host twin and beside dabgpu_packet_slides_dev
on the corrected frames (GPU box).

  python tools/packet_fec_time.py [--streams 64] [--frames 16,256] [--reps 20] [--out profiles/packet_fec_time.txt] [--limit 900]

One visit to the GPU, in a child process that is ended after --limit seconds.  Every sub-channel carries slide data in
packets of four slots inside FEC frames (synth.packet_fec_frames), in three conditions: clean; one packet of every FEC frame
overwritten; four packets of every FEC frame overwritten (8 errors in every row: the bound).  Per batch shape and condition the
child times, over --reps repetitions after two warm-up calls, as stream-synchronised wall time and between two events on the
stream:
  (a) the FEC call, the state records swapped between calls
  (b) the slides call on the frames (a) wrote, the state records swapped, the arena in place
  (c) (a) then (b) on the same stream
  (d) the host twin dabgpu_packet_fec_host on the same table in host memory (wall time, one thread)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

ADDRESS = 7
CONDITIONS = (("clean", 0), ("one damaged packet per FEC frame", 1), ("four damaged packets per FEC frame", 4))


def fec_stream(synth, np, br, n):
    """n logical frames at this bit rate: slides in packets of four slots, in FEC frames from the first slot on"""
    groups = []
    for k in range(max(1, n * (br // 8) * 24 // 9000)):
        data = bytes(np.random.default_rng(br * 1000 + k).integers(0, 256, 8000, dtype=np.uint8))
        groups += synth.mot_object_groups(0x4000 + k, synth.slide_header(len(data), b"slide-%d-%d.jpg" % (br, k)), data, 1024)
    return synth.packet_fec_frames(br, [synth.packetise(groups, ADDRESS, sizes=(4,))], n_frames=n)[:n]


def child(a):
    import numpy as np
    import torch
    import dabgpu
    from dabgpu import synth
    dev = torch.device("cuda", 0)
    prng = np.random.default_rng(2025)
    prates = [int(br) for _ in range(a.streams) for br in prng.choice([32, 64, 128], size=int(prng.integers(1, 3)))]
    lines = ["packet_fec_time: %d ensembles, %d packet sub-channels with FEC frames (%d kbit/s in all, %d..%d each), %s"
             % (a.streams, len(prates), sum(prates), min(prates), max(prates), torch.cuda.get_device_name(0))]
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
            n_cifs = 4 * fps
            clean = {br: fec_stream(synth, np, br, n_cifs + 7) for br in sorted(set(prates))}
            for label, damaged in CONDITIONS:
                keep, fswap, hswap, pswap, fcnts, pcnts = [], [[], []], [[], []], [[], []], [], []
                for e, br in enumerate(prates):
                    host = np.ascontiguousarray(clean[br][e % 7:e % 7 + n_cifs]).copy()
                    flat = host.reshape(-1, 24)
                    rng = np.random.default_rng(e)
                    first = (103 - (e % 7) * (br // 8) % 103) % 103
                    for t in range(first, len(flat) - 102, 103):
                        for s in rng.choice(94, damaged, replace=False):
                            flat[t + s] = rng.integers(0, 256, 24, dtype=np.uint8) | np.uint8(0x40)
                    fb = dabgpu.packet_fec_state_bytes(br)
                    frames = torch.from_numpy(host).to(dev)
                    out = torch.zeros((n_cifs, 3 * br), dtype=torch.uint8, device=dev)
                    f0, f1 = (torch.zeros((fb,), dtype=torch.uint8, device=dev) for _ in range(2))
                    fcnt = torch.zeros((48,), dtype=torch.uint8, device=dev)
                    s0, s1 = (torch.zeros((nb,), dtype=torch.uint8, device=dev) for _ in range(2))
                    arena = torch.zeros((ab,), dtype=torch.uint8, device=dev)
                    slides = torch.zeros((slots, stride), dtype=torch.uint8, device=dev)
                    pcnt = torch.zeros((192,), dtype=torch.uint8, device=dev)
                    h = [np.zeros(fb + 16, np.uint8), np.zeros(fb + 16, np.uint8), np.zeros((n_cifs, 3 * br), np.uint8), np.zeros(48, np.uint8)]
                    al = [x[-x.ctypes.data % 16:] for x in h[:2]]
                    keep += [frames, out, f0, f1, s0, s1, arena, slides, host, h]
                    fcnts.append(fcnt)
                    pcnts.append(pcnt)
                    for side, (si, so) in enumerate(((f0, f1), (f1, f0))):
                        fswap[side].append(dabgpu.PacketFecEntry(frames.data_ptr(), 3 * br, br, 0, out.data_ptr(), 3 * br, si.data_ptr(), so.data_ptr(), fcnt.data_ptr()))
                        hswap[side].append(dabgpu.PacketFecEntry(host.ctypes.data, 3 * br, br, 0, h[2].ctypes.data, 3 * br, al[side].ctypes.data, al[side ^ 1].ctypes.data,
                                                                 h[3].ctypes.data))
                    for side, (si, so) in enumerate(((s0, s1), (s1, s0))):
                        pswap[side].append(dabgpu.PacketEntry(out.data_ptr(), 3 * br, br, ADDRESS, 1, 0, si.data_ptr(), so.data_ptr(), arena.data_ptr(), ab,
                                                              slides.data_ptr(), stride, slots, 0, pcnt.data_ptr()))
                torch.cuda.synchronize()
                turn = [0, 0, 0]

                def fec():
                    ctx.packet_fec_dev(fswap[turn[0]], n_cifs)
                    turn[0] ^= 1

                def packets():
                    ctx.packet_slides_dev(pswap[turn[1]], n_cifs)
                    turn[1] ^= 1

                def both():
                    fec()
                    packets()

                wall_a, dev_a = timed(fec)
                fc = np.stack([c.cpu().numpy().view(dabgpu.PACKET_FEC_RESULT_DTYPE)[0] for c in fcnts])
                wall_b, dev_b = timed(packets)
                wall_c, dev_c = timed(both)
                pc = np.stack([c.cpu().numpy().view(dabgpu.PACKET_RESULT_DTYPE)[0] for c in pcnts])
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    dabgpu.packet_fec_host(hswap[turn[2]], n_cifs)
                    turn[2] ^= 1
                wall_d = (time.perf_counter() - t0) * 1e3 / a.reps
                lines += ["%d x %d frames, %s (%d logical frames per entry; the last FEC call: %d slots, %d FEC frames, rows: %d clean, %d corrected, %d "
                          "uncorrectable; %d data bytes corrected; the last slides call behind it: %d bad slots, %d followed packets, %d continuity breaks):"
                          % (a.streams, fps, label, n_cifs, fc["slots"].sum(), fc["frames"].sum(), fc["rows_clean"].sum(), fc["rows_corrected"].sum(),
                             fc["rows_uncorrectable"].sum(), fc["bytes_corrected"].sum(), pc["slots_bad"].sum(), pc["packets_followed"].sum(),
                             pc["continuity_breaks"].sum()),
                          "  (a) the FEC call                        %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_a, dev_a, a.reps),
                          "  (b) the slides call on its output       %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_b, dev_b, a.reps),
                          "  (c) (a) then (b) on the same stream     %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_c, dev_c, a.reps),
                          "  (d) the host twin of (a), same table    %9.3f ms wall, one thread                               (d) / (a) = %.1f wall" % (wall_d, wall_d / wall_a)]
                del keep, fswap, hswap, pswap, fcnts, pcnts
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packet_fec_time.txt"))
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
        sys.exit("packet_fec_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
