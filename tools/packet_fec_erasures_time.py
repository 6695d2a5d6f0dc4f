#!/usr/bin/env python3
"""Time dabgpu_packet_fec_erasures_dev against dabgpu_packet_fec_dev on the packet-mode sub-channels of
tools/packet_fec_time.py's batch (same seed: 64 ensembles, 94 packet sub-channels of 32, 64 or 128 kbit/s, in FEC frames), and
against its own host twin (GPU box).

  python tools/packet_fec_erasures_time.py [--streams 64] [--frames 16,256] [--rounds 10] [--inner 5]
                                           [--out profiles/packet_fec_erasures_time.txt] [--limit 900]

One visit to the GPU, in a child process that is ended after --limit seconds.  Every sub-channel carries slide data in packets
of ONE slot (tools/packet_fec_time.py's are of four: there an overwritten slot makes four suspect slots, here a lost packet is
one), in three conditions: clean; four packets of every FEC frame overwritten (8 wrong bytes a row: the errors-only bound);
eight (16 erased columns: the erasure bound, where the errors-only call corrects nothing).  Five variants per batch shape:
the errors-only call and the erasure call on clean input, both with four damaged packets, the erasure call with eight.  They
are timed in ONE process in interleaved rounds: --rounds rounds, in each every variant in turn for --inner calls between two
events on the stream, the state records swapped between calls; the median and the minimum over the rounds are reported, and
the ratio of the medians erasure / errors-only.  (As in tools/packet_fec_time.py one call is repeated on the same frames with the
state carried on, so the FEC frames that straddle the seam between two repetitions are no codewords: the uncorrectable rows of
the clean condition are those.  The last tenth of every stream is padding in packets of up to four slots, where an overwritten
slot makes up to four suspect slots: the FEC frames beyond 16 erasures of the eight-packet condition are those.)  The host
twin dabgpu_packet_fec_erasures_host runs the eight-packet table in host memory (wall time, one thread)."""
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
VARIANTS = (("errors-only call, clean", 0, 0), ("erasure call,     clean", 1, 0), ("errors-only call, four damaged packets per FEC frame", 0, 4),
            ("erasure call,     four damaged packets per FEC frame", 1, 4), ("erasure call,     eight damaged packets per FEC frame", 1, 8))


def fec_stream(synth, np, br, n):
    """n logical frames at this bit rate: slides in packets of one slot, in FEC frames from the first slot on"""
    groups = []
    for k in range(max(1, n * (br // 8) * 19 // 9000)):
        data = bytes(np.random.default_rng(br * 1000 + k).integers(0, 256, 8000, dtype=np.uint8))
        groups += synth.mot_object_groups(0x4000 + k, synth.slide_header(len(data), b"slide-%d-%d.jpg" % (br, k)), data, 1024)
    return synth.packet_fec_frames(br, [synth.packetise(groups, ADDRESS, sizes=(1,))], n_frames=n)[:n]


def child(a):
    import numpy as np
    import torch
    import dabgpu
    from dabgpu import synth
    dev = torch.device("cuda", 0)
    prng = np.random.default_rng(2025)
    prates = [int(br) for _ in range(a.streams) for br in prng.choice([32, 64, 128], size=int(prng.integers(1, 3)))]
    lines = ["packet_fec_erasures_time: %d ensembles, %d packet sub-channels with FEC frames (%d kbit/s in all, %d..%d each), %s"
             % (a.streams, len(prates), sum(prates), min(prates), max(prates), torch.cuda.get_device_name(0)),
             "interleaved rounds in one process: %d rounds x %d calls per variant; ms per call between events, median (minimum)" % (a.rounds, a.inner)]
    with dabgpu.Context(device=0, max_frames=64) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        for fps in a.frames:
            n_cifs = 4 * fps
            clean = {br: fec_stream(synth, np, br, n_cifs + 7) for br in sorted(set(prates))}
            keep, runs, results, host_tables = [], [], [], None
            for label, erasures, damaged in VARIANTS:
                swap, cnts, hswap = [[], []], [], [[], []]
                Entry = dabgpu.PacketFecErasureEntry if erasures else dabgpu.PacketFecEntry
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
                    cnt = torch.zeros((80,), dtype=torch.uint8, device=dev)
                    keep += [frames, out, f0, f1, host]
                    cnts.append(cnt)
                    for side, (si, so) in enumerate(((f0, f1), (f1, f0))):
                        swap[side].append(Entry(frames.data_ptr(), 3 * br, br, 0, out.data_ptr(), 3 * br, si.data_ptr(), so.data_ptr(), cnt.data_ptr()))
                    if damaged == 8:
                        h = [np.zeros(fb + 16, np.uint8), np.zeros(fb + 16, np.uint8), np.zeros((n_cifs, 3 * br), np.uint8), np.zeros(80, np.uint8)]
                        al = [x[-x.ctypes.data % 16:] for x in h[:2]]
                        keep.append(h)
                        for side in range(2):
                            hswap[side].append(Entry(host.ctypes.data, 3 * br, br, 0, h[2].ctypes.data, 3 * br, al[side].ctypes.data, al[side ^ 1].ctypes.data,
                                                     h[3].ctypes.data))
                call = ctx.packet_fec_erasures_dev if erasures else ctx.packet_fec_dev
                turn = [0]

                def run(call=call, swap=swap, turn=turn):
                    call(swap[turn[0]], n_cifs)
                    turn[0] ^= 1

                runs.append(run)
                results.append(cnts)
                if damaged == 8:
                    host_tables = hswap
            torch.cuda.synchronize()
            for run in runs:
                run()
                run()
            ctx.sync()
            times = [[] for _ in runs]
            for _ in range(a.rounds):
                for k, run in enumerate(runs):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.inner):
                        run()
                    e1.record(stream)
                    ctx.sync()
                    times[k].append(e0.elapsed_time(e1) / a.inner)
            med = [float(np.median(t)) for t in times]
            lines.append("%d x %d frames (%d logical frames per entry):" % (a.streams, fps, n_cifs))
            for k, (label, erasures, damaged) in enumerate(VARIANTS):
                dt = dabgpu.PACKET_FEC_ERASURE_RESULT_DTYPE if erasures else dabgpu.PACKET_FEC_RESULT_DTYPE
                c = np.stack([x.cpu().numpy()[:dt.itemsize].view(dt)[0] for x in results[k]])
                tail = ", %d by erasures, %d suspect slots, %d FEC frames beyond 16 erasures" % (c["rows_erasure_corrected"].sum(), c["slots_suspect"].sum(),
                                                                                                   c["frames_beyond_erasures"].sum()) if erasures else ""
                lines.append("  %-55s %9.3f (%9.3f) ms   last call: %d FEC frames, rows: %d clean, %d corrected, %d uncorrectable%s"
                             % (label, med[k], min(times[k]), c["frames"].sum(), c["rows_clean"].sum(), c["rows_corrected"].sum(), c["rows_uncorrectable"].sum(), tail))
            lines.append("  erasure / errors-only, medians: clean %.2f, four damaged packets %.2f" % (med[1] / med[0], med[3] / med[2]))
            reps, turn = 3, 0
            t0 = time.perf_counter()
            for _ in range(reps):
                dabgpu.packet_fec_erasures_host(host_tables[turn], n_cifs)
                turn ^= 1
            wall = (time.perf_counter() - t0) * 1e3 / reps
            lines.append("  host twin of the erasure call, eight damaged packets    %9.3f ms wall, one thread (mean of %d): %.0f x the device call"
                         % (wall, reps, wall / med[4]))
            del keep, runs, results, host_tables
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", default="16,256", help="frames per stream, one batch shape each")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packet_fec_erasures_time.txt"))
    ap.add_argument("--limit", type=int, default=900, help="seconds the GPU visit may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        a.frames = [int(x) for x in a.frames.split(",")]
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--streams", str(a.streams), "--frames", a.frames, "--rounds", str(a.rounds),
           "--inner", str(a.inner), "--out", a.out]
    try:
        sys.exit(subprocess.run(cmd, timeout=a.limit).returncode)
    except subprocess.TimeoutExpired:
        sys.exit("packet_fec_erasures_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
