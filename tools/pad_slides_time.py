#!/usr/bin/env python3
"""Time dabgpu_mot_slides_dev beside dabgpu_pad_labels_dev and dabgpu_dabplus_follow_dev on the DAB+ entries of a batch of
ensembles (GPU box).

  python tools/pad_slides_time.py [--streams 64] [--frames 16,256] [--reps 20] [--out profiles/pad_slides_time.txt] [--limit 900]

One visit to the GPU, in a child process that is ended after --limit seconds.  The workload is that of
tools/pad_labels_time.py (same plans, same seed), with every access unit's X-PAD as full of slide data as the unit has room
for, beside a label sub-field: each entry's four-super-frame cycle carries two slideshow objects (two transport ids, so
that each of them completes in every cycle) sized to what the cycle holds, and a three-segment dynamic label.  Per batch
shape the child times, over --reps repetitions after two warm-up calls, as stream-synchronised wall time and between two
events on the stream:
  (a) the follow call alone, the carry records swapped between calls
  (b) the label call alone, on what the last follow call left, the state records swapped between calls
  (c) the slide call alone, likewise, the arena in place
  (d) all three in sequence on the same stream: what a monitoring receiver pays per batch
and a plain device-to-device copy of as many bytes as the slide call moved, the yardstick for (c) - (b)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def cycle_bodies(synth, np, br, text):
    """the twelve access units of a cycle at this bit rate: label and two objects as large as the cycle has room for"""
    size = 110 * br // 8
    cuts = [6 + a_ * (size - 6) // 3 for a_ in (1, 2)]
    sizes = [b - a_ for a_, b in zip([6] + cuts, cuts + [size])] * 4
    label = synth.dls_segments(text, 0)
    body = max(sum(min(n - 11, 190) for n in sizes) - 12 * 12, 0)
    while True:
        groups = []
        for k in range(2):
            data = bytes(np.random.default_rng(br * 2 + k).integers(0, 256, body // 2, dtype=np.uint8))
            groups += synth.mot_object_groups(0x4000 + 2 * br + k, synth.slide_header(len(data), b"slide-%d-%d.jpg" % (br, k)), data, 1024)
        pads, left = synth.pack_pads(sizes, groups, label, dls_index=3 if size >= 200 else 0)
        if left == 0 or body == 0:
            break
        body = body * 9 // 10 if body > 40 else 0
    if left:                                                          # too small for a slide: the label alone
        pads, left = synth.pack_pads(sizes, [], label, dls_index=0)
    return cuts, [[synth.au_body(p) if p is not None else b"\x21" for p in pads[3 * q:3 * q + 3]] for q in range(4)], body


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
    lines = ["pad_slides_time: %d ensembles, %d DAB+ entries (%d kbit/s in all, %d..%d each), X-PAD full of slide data beside a label in every "
             "access unit, %s" % (a.streams, len(rates), sum(rates), min(rates), max(rates), torch.cuda.get_device_name(0))]
    text = b"Now playing: Some Artist - The Title Of A Song"[:44]
    cycle, carried = {}, {}
    for br in sorted(set(rates)):
        cuts, bodies, carried[br] = cycle_bodies(synth, np, br, text)
        cycle[br] = np.concatenate([synth.build_superframe(rng, br, 1, 1, cuts=cuts, bodies=bodies[q])[0] for q in range(4)]).reshape(20, 3 * br)
    lines.append("slide bytes per cycle of four super-frames, by bit rate: " + ", ".join("%d: %d" % (br, carried[br]) for br in sorted(carried)))
    nb, mb, cap, stride, slots = dabgpu.pad_state_bytes(), dabgpu.mot_state_bytes(), 4096, 4096 + 256, 4
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
            keep, swap, pswap, mswap, cnts, mcnts = [], [[], []], [[], []], [[], []], [], []
            for e, br in enumerate(rates):
                s, off = br // 8, e % 5
                frames = torch.from_numpy(np.ascontiguousarray(cycle[br][(np.arange(n_cifs) - off) % 20])).to(dev)
                data = torch.zeros((max_sf, 110 * s), dtype=torch.uint8, device=dev)
                st = torch.zeros((max_sf * 64,), dtype=torch.uint8, device=dev)
                res = torch.zeros((32,), dtype=torch.uint8, device=dev)
                c0, c1 = (torch.zeros((dabgpu.dabplus_carry_bytes(br),), dtype=torch.uint8, device=dev) for _ in range(2))
                s0, s1 = (torch.zeros((nb,), dtype=torch.uint8, device=dev) for _ in range(2))
                m0, m1 = (torch.zeros((mb,), dtype=torch.uint8, device=dev) for _ in range(2))
                arena = torch.zeros((ab,), dtype=torch.uint8, device=dev)
                slides = torch.zeros((slots, stride), dtype=torch.uint8, device=dev)
                lab = torch.zeros((144,), dtype=torch.uint8, device=dev)
                cnt = torch.zeros((64,), dtype=torch.uint8, device=dev)
                mcnt = torch.zeros((128,), dtype=torch.uint8, device=dev)
                keep += [frames, data, st, res, c0, c1, s0, s1, m0, m1, arena, slides, lab]
                cnts.append(cnt)
                mcnts.append(mcnt)
                for side, (ci, co, si, so, mi, mo) in enumerate(((c0, c1, s0, s1, m0, m1), (c1, c0, s1, s0, m1, m0))):
                    swap[side].append(dabgpu.DabplusEntry(frames.data_ptr(), 3 * br, br, ci.data_ptr(), co.data_ptr(), data.data_ptr(),
                                                          st.data_ptr(), res.data_ptr()))
                    pswap[side].append(dabgpu.PadEntry(data.data_ptr(), 110 * s, st.data_ptr(), res.data_ptr(), br, max_sf, si.data_ptr(),
                                                       so.data_ptr(), lab.data_ptr(), cnt.data_ptr()))
                    mswap[side].append(dabgpu.MotEntry(data.data_ptr(), 110 * s, st.data_ptr(), res.data_ptr(), br, max_sf, mi.data_ptr(),
                                                       mo.data_ptr(), arena.data_ptr(), ab, slides.data_ptr(), stride, slots, 0, mcnt.data_ptr()))
            torch.cuda.synchronize()
            turn = [0, 0, 0]

            def follow():
                ctx.dabplus_follow_dev(swap[turn[0]], n_cifs)
                turn[0] ^= 1

            def labels():
                ctx.pad_labels_dev(pswap[turn[1]])
                turn[1] ^= 1

            def slides_call():
                ctx.mot_slides_dev(mswap[turn[2]])
                turn[2] ^= 1

            def all_three():
                follow()
                labels()
                slides_call()

            wall_a, dev_a = timed(follow)
            wall_b, dev_b = timed(labels)
            wall_c, dev_c = timed(slides_call)
            wall_d, dev_d = timed(all_three)
            counts = np.stack([c.cpu().numpy().view(dabgpu.PAD_RESULT_DTYPE)[0] for c in cnts])
            mc = np.stack([c.cpu().numpy().view(dabgpu.MOT_RESULT_DTYPE)[0] for c in mcnts])
            moved = int(mc["xpad_bytes"].sum()) + int(mc["object_bytes"].sum())
            src, dst = (torch.zeros((max(moved, 16),), dtype=torch.uint8, device=dev) for _ in range(2))
            with torch.cuda.stream(stream):
                wall_e, dev_e = timed(lambda: dst.copy_(src))
            lines += ["%d x %d frames (%d logical frames per entry; the last slide call walked %d access units, %d with X-PAD; %d groups ok, %d CRC "
                      "failed, %d malformed; %d segments placed, %d objects completed, %d slides written, %d dropped; %d X-PAD bytes into data "
                      "groups, %d bytes into objects and slots; the last label call: %d groups):" %
                      (a.streams, fps, n_cifs, mc["aus"].sum(), mc["aus_with_xpad"].sum(), mc["groups_ok"].sum(), mc["groups_crc_failed"].sum(),
                       mc["groups_malformed"].sum() + mc["pad_malformed"].sum(), mc["segments_placed"].sum(), mc["objects_completed"].sum(),
                       mc["slides_written"].sum(), mc["slides_dropped"].sum(), mc["xpad_bytes"].sum(), mc["object_bytes"].sum(), counts["groups_ok"].sum()),
                      "  (a) the follow call alone       %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_a, dev_a, a.reps),
                      "  (b) the label call alone        %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_b, dev_b, a.reps),
                      "  (c) the slide call alone        %9.3f ms wall  %9.3f ms between events  (mean of %d)   (c) / (b) = %.2f wall, %.2f events"
                      % (wall_c, dev_c, a.reps, wall_c / wall_b, dev_c / dev_b),
                      "  (d) all three in sequence       %9.3f ms wall  %9.3f ms between events  (mean of %d)   (d) / (a) = %.2f wall, %.2f events"
                      % (wall_d, dev_d, a.reps, wall_d / wall_a, dev_d / dev_a),
                      "      a plain device copy of the %d bytes moved: %.3f ms wall  %.3f ms between events; (c) - (b) = %.3f ms between events"
                      % (moved, wall_e, dev_e, dev_c - dev_b)]
            del keep, swap, pswap, mswap, cnts, mcnts
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pad_slides_time.txt"))
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
        sys.exit("pad_slides_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
