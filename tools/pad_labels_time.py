#!/usr/bin/env python3
"""Time dabgpu_pad_labels_dev beside dabgpu_dabplus_follow_dev on the DAB+ entries of a batch of ensembles (GPU box).

  python tools/pad_labels_time.py [--streams 64] [--frames 16,256] [--reps 20] [--out profiles/pad_labels_time.txt] [--limit 600]

One visit to the GPU, in a child process that is ended after --limit seconds.  The workload is that of
tools/dabplus_follow_time.py (same plans, same seed), with PAD in EVERY access unit: each entry's four-super-frame cycle
carries a three-segment dynamic label in variable X-PAD sub-fields of 12 bytes, one per access unit, so every access unit
costs the walk a content-indicator list, a sub-field and its share of a data group.  Per batch shape the child times, over
--reps repetitions after two warm-up calls, as stream-synchronised wall time and between two events on the stream:
  (a) the follow call alone, the carry records swapped between calls
  (b) the label call alone, on what the last follow call left, the state records swapped between calls
  (c) both, the label call behind the follow call on the same stream: what a monitoring receiver pays per batch"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


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
    lines = ["pad_labels_time: %d ensembles, %d DAB+ entries (%d kbit/s in all, %d..%d each), PAD in every access unit, %s" %
             (a.streams, len(rates), sum(rates), min(rates), max(rates), torch.cuda.get_device_name(0))]
    text = b"Now playing: Some Artist - The Title Of A Song"[:44]
    pads = synth.dls_pads(synth.dls_segments(text, 0) + synth.dls_segments(text, 0), length_index=3)
    assert len(pads) == 12
    bodies = [[synth.au_body(p) for p in pads[3 * q:3 * q + 3]] for q in range(4)]
    cycle = {}
    for br in sorted(set(rates)):
        size = 110 * br // 8
        cuts = [6 + a_ * (size - 6) // 3 for a_ in (1, 2)]
        cycle[br] = np.concatenate([synth.build_superframe(rng, br, 1, 1, cuts=cuts, bodies=bodies[q])[0] for q in range(4)]).reshape(20, 3 * br)
    nb = dabgpu.pad_state_bytes()

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
            keep, swap, pswap = [], [[], []], [[], []]
            for e, br in enumerate(rates):
                s, off = br // 8, e % 5
                frames = torch.from_numpy(np.ascontiguousarray(cycle[br][(np.arange(n_cifs) - off) % 20])).to(dev)
                data = torch.zeros((max_sf, 110 * s), dtype=torch.uint8, device=dev)
                st = torch.zeros((max_sf * 64,), dtype=torch.uint8, device=dev)
                res = torch.zeros((32,), dtype=torch.uint8, device=dev)
                c0, c1 = (torch.zeros((dabgpu.dabplus_carry_bytes(br),), dtype=torch.uint8, device=dev) for _ in range(2))
                s0, s1 = (torch.zeros((nb,), dtype=torch.uint8, device=dev) for _ in range(2))
                lab = torch.zeros((144,), dtype=torch.uint8, device=dev)
                cnt = torch.zeros((64,), dtype=torch.uint8, device=dev)
                keep += [frames, data, st, res, c0, c1, s0, s1, lab, cnt]
                for side, (ci, co, si, so) in enumerate(((c0, c1, s0, s1), (c1, c0, s1, s0))):
                    swap[side].append(dabgpu.DabplusEntry(frames.data_ptr(), 3 * br, br, ci.data_ptr(), co.data_ptr(), data.data_ptr(),
                                                          st.data_ptr(), res.data_ptr()))
                    pswap[side].append(dabgpu.PadEntry(data.data_ptr(), 110 * s, st.data_ptr(), res.data_ptr(), br, max_sf, si.data_ptr(),
                                                       so.data_ptr(), lab.data_ptr(), cnt.data_ptr()))
            torch.cuda.synchronize()
            turn = [0, 0]

            def follow():
                ctx.dabplus_follow_dev(swap[turn[0]], n_cifs)
                turn[0] ^= 1

            def labels():
                ctx.pad_labels_dev(pswap[turn[1]])
                turn[1] ^= 1

            def both():
                follow()
                labels()

            wall_a, dev_a = timed(follow)
            wall_b, dev_b = timed(labels)
            wall_c, dev_c = timed(both)
            counts = np.stack([keep[10 * e + 9].cpu().numpy().view(dabgpu.PAD_RESULT_DTYPE)[0] for e in range(len(rates))])
            shown = sum(bytes(keep[10 * e + 8].cpu().numpy()[16:16 + len(text)]) == text for e in range(len(rates)))
            lines += ["%d x %d frames (%d logical frames per entry; the last label call walked %d access units, %d with X-PAD, %d groups, "
                      "%d malformed; %d of %d entries show the label):" % (a.streams, fps, n_cifs, counts["aus"].sum(), counts["aus_with_xpad"].sum(),
                                                                            counts["groups_ok"].sum(), counts["pad_malformed"].sum(), shown, len(rates)),
                      "  (a) the follow call alone       %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_a, dev_a, a.reps),
                      "  (b) the label call alone        %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_b, dev_b, a.reps),
                      "  (c) the label call behind it    %9.3f ms wall  %9.3f ms between events  (mean of %d)   (c) / (a) = %.2f wall, %.2f events"
                      % (wall_c, dev_c, a.reps, wall_c / wall_a, dev_c / dev_a)]
            del keep, swap, pswap
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pad_labels_time.txt"))
    ap.add_argument("--limit", type=int, default=600, help="seconds the GPU visit may take")
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
        sys.exit("pad_labels_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
