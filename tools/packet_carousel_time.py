#!/usr/bin/env python3
"""Time dabgpu_packet_carousel_dev on the packet-mode sub-channels of a batch of ensembles against dabgpu_packet_slides_dev
on the same objects, and against the host twin on the same table (GPU box).

  python tools/packet_carousel_time.py [--streams 64] [--frames 16,256] [--reps 10] [--rounds 4] [--out profiles/packet_carousel_time.txt] [--limit 900]

One visit to the GPU, in a child process that is ended after --limit seconds.  The sub-channels are those of
tools/packet_slides_time.py (same seed: one or two of 32, 64 or 128 kbit/s per ensemble), each as full of object data as
20 frames have room for: two objects (two transport ids) in packets of four slots of one address, and in the next 20 frames
the same bytes under two other transport ids, a cycle of 40.  The SAME objects are sent twice: once in header mode (type-3
header groups, then bodies) for dabgpu_packet_slides_dev, and once as directory carousels (a type-6 directory that lists
the two objects of its half, then the bodies; the other half under another directory id, so that the directory changes and
its objects are delivered again in every half, as the slides call delivers them) for dabgpu_packet_carousel_dev.  Per batch shape
the child times, in --rounds interleaved rounds of --reps calls each after two warm-up calls, as stream-synchronised wall
time and between two events on the stream:
  (s) the slides call on the header-mode frames, the state records swapped, the arena in place: the yardstick
  (n) the carousel call with an address no packet carries: the scan launch, and a walk launch that only sums the scan's records
  (c) the carousel call on the carousel frames, the state records swapped, the arena in place
  (h) the host twins of (s) and (c) on the same tables in host memory (wall time, one thread)
Every round runs (s), (n), (c) in that order, so drift of the clock meets all three alike; the mean and the best round of each
are reported."""
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
    """40 logical frames of a packet sub-channel at this bit rate, as full of objects as they get, in both modes: two halves of
    20 frames with two objects each, the second half the same bytes under other transport ids (and, in directory mode, under
    another directory id), so that every half delivers its two objects in either mode for as long as the cycle repeats ->
    (header-mode frames, carousel frames, body bytes per half)"""
    body = 20 * (br // 8) * 24 * 9 // 10
    while True:
        out = [[], []]
        for half in range(2):
            objs = []
            for k in range(2):
                data = bytes(np.random.default_rng(br * 2 + k).integers(0, 256, body // 2, dtype=np.uint8))
                objs.append((0x4000 + 4 * br + 2 * half + k, synth.slide_header(len(data), b"logo-%d-%d.png" % (br, k)), data))
            header_mode = [g for tid, h, data in objs for g in synth.mot_object_groups(tid, h, data, 1024)]
            d, bodies = synth.mot_carousel_groups(0x3000 + 2 * br + half, objs, 1024)
            for m, groups in enumerate((header_mode, d + [g for b in bodies for g in b])):
                packets = synth.packetise(groups, ADDRESS, sizes=(4,))
                while len(packets) % 4:
                    packets.append(synth.packet(ADDRESS, b"\x00", 1, ci=len(packets), command=True))
                out[m].append(synth.packet_frames(br, [packets], n_frames=20))
        if all(len(f) == 20 for m in out for f in m):
            return np.concatenate(out[0]), np.concatenate(out[1]), body
        body = body * 19 // 20


def child(a):
    import numpy as np
    import torch
    import dabgpu
    from dabgpu import synth
    dev = torch.device("cuda", 0)
    prng = np.random.default_rng(2025)
    prates = [int(br) for _ in range(a.streams) for br in prng.choice([32, 64, 128], size=int(prng.integers(1, 3)))]
    lines = ["packet_carousel_time: %d ensembles, %d packet sub-channels (%d kbit/s in all, %d..%d each) full of object data, %s"
             % (a.streams, len(prates), sum(prates), min(prates), max(prates), torch.cuda.get_device_name(0))]
    cycle, carried = {}, {}
    for br in sorted(set(prates)):
        h, c, carried[br] = cycle_frames(synth, np, br)
        cycle[br] = (h, c)
    lines.append("object bytes per half cycle of 20 logical frames, by bit rate: " + ", ".join("%d: %d" % (br, carried[br]) for br in sorted(carried)))
    cap, stride, slots = 8192, 8192 + 1024 + 256, 128      # (slots for every object of the longest call)
    sizes = (1024, 4, cap)
    nb_s, nb_c = dabgpu.packet_state_bytes(), dabgpu.packet_carousel_state_bytes()
    ab_s, ab_c = dabgpu.mot_arena_bytes(cap), dabgpu.packet_carousel_arena_bytes(*sizes)
    lines.append("carousel entries: directory_capacity %d, assemblies %d, object_capacity %d; state record %d bytes (slides: %d), arena %d bytes (slides: %d)"
                 % (sizes + (nb_c, nb_s, ab_c, ab_s)))

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

        def aligned(n):
            raw = np.zeros(n + 16, np.uint8)
            return raw[-raw.ctypes.data % 16:][:n]

        for fps in a.frames:
            n_cifs = 4 * fps
            keep, sswap, cswap, nobody, hs, hc, scnt, ccnt = [], [[], []], [[], []], [], [[], []], [[], []], [], []
            for e, br in enumerate(prates):
                pick = (np.arange(n_cifs) - e % 7) % 40
                host = [np.ascontiguousarray(cycle[br][m][pick]) for m in range(2)]
                frames = [torch.from_numpy(x).to(dev) for x in host]
                st = [torch.zeros((nb,), dtype=torch.uint8, device=dev) for nb in (nb_s, nb_s, nb_c, nb_c, nb_c)]
                arena = [torch.zeros((ab,), dtype=torch.uint8, device=dev) for ab in (ab_s, ab_c)]
                out = [torch.zeros((slots, stride), dtype=torch.uint8, device=dev) for _ in range(2)]
                directory = torch.zeros((sizes[0],), dtype=torch.uint8, device=dev)
                cnt = [torch.zeros((n,), dtype=torch.uint8, device=dev) for n in (192, 256)]
                hb = [aligned(nb_s), aligned(nb_s), aligned(nb_c), aligned(nb_c), aligned(ab_s), aligned(ab_c), aligned(slots * stride), aligned(slots * stride),
                      aligned(sizes[0]), aligned(192), aligned(256)]
                keep += [host, frames, st, arena, out, directory, cnt, hb]
                scnt.append(cnt[0])
                ccnt.append(cnt[1])
                for side in range(2):
                    sswap[side].append(dabgpu.PacketEntry(frames[0].data_ptr(), 3 * br, br, ADDRESS, 0, 0, st[side].data_ptr(), st[side ^ 1].data_ptr(),
                                                          arena[0].data_ptr(), ab_s, out[0].data_ptr(), stride, slots, 0, cnt[0].data_ptr()))
                    cswap[side].append(dabgpu.PacketCarouselEntry(frames[1].data_ptr(), 3 * br, br, ADDRESS, 0, sizes[1], st[2 + side].data_ptr(),
                                                                  st[2 + (side ^ 1)].data_ptr(), arena[1].data_ptr(), ab_c, out[1].data_ptr(), stride, slots,
                                                                  sizes[2], directory.data_ptr(), sizes[0], 0, cnt[1].data_ptr()))
                    hs[side].append(dabgpu.PacketEntry(host[0].ctypes.data, 3 * br, br, ADDRESS, 0, 0, hb[side].ctypes.data, hb[side ^ 1].ctypes.data,
                                                       hb[4].ctypes.data, ab_s, hb[6].ctypes.data, stride, slots, 0, hb[9].ctypes.data))
                    hc[side].append(dabgpu.PacketCarouselEntry(host[1].ctypes.data, 3 * br, br, ADDRESS, 0, sizes[1], hb[2 + side].ctypes.data,
                                                               hb[2 + (side ^ 1)].ctypes.data, hb[5].ctypes.data, ab_c, hb[7].ctypes.data, stride, slots,
                                                               sizes[2], hb[8].ctypes.data, sizes[0], 0, hb[10].ctypes.data))
                nobody.append(dabgpu.PacketCarouselEntry(frames[1].data_ptr(), 3 * br, br, NOBODY, 0, sizes[1], None, st[4].data_ptr(), arena[1].data_ptr(), ab_c,
                                                         out[1].data_ptr(), stride, slots, sizes[2], directory.data_ptr(), sizes[0], 0, cnt[1].data_ptr()))
            torch.cuda.synchronize()
            turn = [0, 0, 0, 0]

            def slides():
                ctx.packet_slides_dev(sswap[turn[0]], n_cifs)
                turn[0] ^= 1

            def carousel():
                ctx.packet_carousel_dev(cswap[turn[1]], n_cifs)
                turn[1] ^= 1

            rounds = {"s": [], "n": [], "c": []}
            for _ in range(a.rounds):
                rounds["s"].append(timed(slides))
                rounds["n"].append(timed(lambda: ctx.packet_carousel_dev(nobody, n_cifs)))
                rounds["c"].append(timed(carousel))
            sc = np.stack([c.cpu().numpy().view(dabgpu.PACKET_RESULT_DTYPE)[0] for c in scnt])
            cc = np.stack([c.cpu().numpy().view(dabgpu.PACKET_CAROUSEL_RESULT_DTYPE)[0] for c in ccnt])
            host_ms = []
            for run, table, k in ((dabgpu.packet_slides_host, hs, 2), (dabgpu.packet_carousel_host, hc, 3)):
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    run(table[turn[k]], n_cifs)
                    turn[k] ^= 1
                host_ms.append((time.perf_counter() - t0) * 1e3 / a.reps)

            def stat(key):
                wall, evt = [w for w, _ in rounds[key]], [e for _, e in rounds[key]]
                return sum(wall) / len(wall), sum(evt) / len(evt), min(evt)

            s, n, c = stat("s"), stat("n"), stat("c")
            lines += ["%d x %d frames (%d logical frames per entry, %d entries).  The last slides call: %d followed packets, %d groups ok, %d segments placed, "
                      "%d slides written, %d dropped, %d + %d bytes moved.  The last carousel call: %d followed packets, %d groups ok (%d repeated), %d segments "
                      "placed, %d directories completed, %d objects written, %d deferred, %d + %d bytes moved:" %
                      (a.streams, fps, n_cifs, len(prates), sc["packets_followed"].sum(), sc["mot"]["groups_ok"].sum(), sc["mot"]["segments_placed"].sum(),
                       sc["mot"]["slides_written"].sum(), sc["mot"]["slides_dropped"].sum(), sc["group_bytes"].sum(), sc["mot"]["object_bytes"].sum(),
                       cc["head"]["packets_followed"].sum(), cc["head"]["mot"]["groups_ok"].sum(), cc["head"]["mot"]["groups_repeated"].sum(),
                       cc["head"]["mot"]["segments_placed"].sum(), cc["directories_completed"].sum(), cc["objects_written"].sum(), cc["objects_deferred"].sum(),
                       cc["head"]["group_bytes"].sum(), cc["head"]["mot"]["object_bytes"].sum()),
                      "  (s) the slides call, header mode          %9.3f ms wall  %9.3f ms between events (best round %.3f)  (mean of %d rounds of %d)" % (s + (a.rounds, a.reps)),
                      "  (n) carousel: scan + nothing to follow    %9.3f ms wall  %9.3f ms between events (best round %.3f)" % n,
                      "  (c) the carousel call, directory mode     %9.3f ms wall  %9.3f ms between events (best round %.3f)   (c) / (s) = %.2f events; (c) - (n) = %.3f ms: the walk's packets"
                      % (c + (c[1] / s[1], c[1] - n[1])),
                      "  (h) the host twins on the same tables: slides %.3f ms, carousel %.3f ms wall, one thread   carousel host / (c) = %.1f wall"
                      % (host_ms[0], host_ms[1], host_ms[1] / c[0])]
            del keep, sswap, cswap, nobody, hs, hc, scnt, ccnt
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", default="16,256", help="frames per stream, one batch shape each")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packet_carousel_time.txt"))
    ap.add_argument("--limit", type=int, default=900, help="seconds the GPU visit may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        a.frames = [int(x) for x in a.frames.split(",")]
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--streams", str(a.streams), "--frames", a.frames, "--reps", str(a.reps),
           "--rounds", str(a.rounds), "--out", a.out]
    try:
        sys.exit(subprocess.run(cmd, timeout=a.limit).returncode)
    except subprocess.TimeoutExpired:
        sys.exit("packet_carousel_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
