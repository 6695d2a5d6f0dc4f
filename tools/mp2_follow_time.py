#!/usr/bin/env python3
"""Time dabgpu_mp2_follow_dev on the layer-II entries of a batch of ensembles, beside dabgpu_dabplus_follow_dev on its DAB+
entries (GPU box).

  python tools/mp2_follow_time.py [--streams 64] [--frames 16,256] [--reps 20] [--out profiles/mp2_follow_time.txt] [--limit 600]
                                  [--commit <what the file says it was measured on>]

One visit to the GPU, in a child process that is ended after --limit seconds.  The plans are those of
tools/dabplus_follow_time.py and tools/pad_labels_time.py (same seed): their UEP sub-channels are the layer-II entries,
their EEP sub-channels the DAB+ entries.  Every layer-II entry repeats a cycle of 20 frames at 48 kHz with the ISO CRC and
a dynamic label in the PAD of every frame; every DAB+ entry a four-super-frame cycle.  Per batch shape the child times, over
--reps repetitions after two warm-up calls, as stream-synchronised wall time and between two events on the stream:
  (a) the DAB+ follow call alone, on the DAB+ entries, the carry records swapped between calls
  (b) the layer-II follow call alone, on the layer-II entries, likewise
  (c) the layer-II follow call and the label call over its rows behind it on the same stream
No time is fixed in advance: the file records what was measured, and on what."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def commit_name():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=10)
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, timeout=10)
        if head.returncode == 0:
            return head.stdout.strip() + (" with local changes" if dirty.stdout.strip() else "")
    except (OSError, subprocess.TimeoutExpired):
        pass
    return "unknown (no git here)"


def child(a):
    import numpy as np
    import torch
    import dabgpu
    from dabgpu import synth
    from ensembles_time import random_plan
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2024)
    plans = [random_plan(dabgpu, rng) for _ in range(a.streams)]
    plus = [sc.bitrate_kbps for p in plans for sc in p if not sc.is_uep]
    mp2 = [sc.bitrate_kbps for p in plans for sc in p if sc.is_uep]
    lines = ["mp2_follow_time: measured on %s, %s" % (a.commit, torch.cuda.get_device_name(0)),
             "%d ensembles: %d layer-II entries (%d kbit/s in all, %d..%d each), %d DAB+ entries (%d kbit/s in all, %d..%d each)" %
             (a.streams, len(mp2), sum(mp2), min(mp2), max(mp2), len(plus), sum(plus), min(plus), max(plus))]
    text = b"Now playing: Some Artist - The Title Of A Song"[:44]
    pads = synth.dls_pads(synth.dls_segments(text, 0), length_index=3)
    cycle2, cycle_plus = {}, {}
    for br in sorted(set(mp2)):
        mode = synth.MP2_MONO if br in (32, 48, 56, 80) else synth.MP2_STEREO
        cycle2[br] = np.stack([synth.mp2_frame(rng, br, mode=mode, pad=pads[k % len(pads)]) for k in range(20)])
    for br in sorted(set(plus)):
        cycle_plus[br] = np.concatenate([synth.build_superframe(rng, br, 1, 1)[0] for _q in range(4)]).reshape(20, 3 * br)
    nb = dabgpu.pad_state_bytes()
    zeros = lambda n: torch.zeros((n,), dtype=torch.uint8, device=dev)

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
            keep, swap_plus, swap2, pswap, outs = [], [[], []], [[], []], [[], []], []
            for e, br in enumerate(plus):
                frames = torch.from_numpy(np.ascontiguousarray(cycle_plus[br][(np.arange(n_cifs) - e % 5) % 20])).to(dev)
                data, st, res = zeros(max_sf * 110 * br // 8), zeros(max_sf * 64), zeros(32)
                c0, c1 = zeros(dabgpu.dabplus_carry_bytes(br)), zeros(dabgpu.dabplus_carry_bytes(br))
                keep += [frames, data, st, res, c0, c1]
                for side, (ci, co) in enumerate(((c0, c1), (c1, c0))):
                    swap_plus[side].append(dabgpu.DabplusEntry(frames.data_ptr(), 3 * br, br, ci.data_ptr(), co.data_ptr(), data.data_ptr(),
                                                               st.data_ptr(), res.data_ptr()))
            for e, br in enumerate(mp2):
                frames = torch.from_numpy(np.ascontiguousarray(cycle2[br][(np.arange(n_cifs) - e % 7) % 20])).to(dev)
                rows, st, fo, res = zeros((n_cifs + 1) * 220), zeros((n_cifs + 1) * 64), zeros(32), zeros(64)
                c0, c1 = zeros(dabgpu.mp2_carry_bytes(br)), zeros(dabgpu.mp2_carry_bytes(br))
                s0, s1, lab, cnt = zeros(nb), zeros(nb), zeros(144), zeros(64)
                keep += [frames, rows, st, fo, c0, c1, s0, s1]
                outs.append((res, lab, cnt))
                for side, (ci, co, si, so) in enumerate(((c0, c1, s0, s1), (c1, c0, s1, s0))):
                    swap2[side].append(dabgpu.Mp2Entry(frames.data_ptr(), 3 * br, br, ci.data_ptr(), co.data_ptr(), rows.data_ptr(), st.data_ptr(),
                                                       fo.data_ptr(), res.data_ptr()))
                    pswap[side].append(dabgpu.PadEntry(rows.data_ptr(), dabgpu.MP2_ROW_BYTES, st.data_ptr(), fo.data_ptr(), dabgpu.MP2_PAD_KBPS,
                                                       n_cifs + 1, si.data_ptr(), so.data_ptr(), lab.data_ptr(), cnt.data_ptr()))
            torch.cuda.synchronize()
            turn = [0, 0, 0]

            def follow_plus():
                ctx.dabplus_follow_dev(swap_plus[turn[0]], n_cifs)
                turn[0] ^= 1

            def follow_mp2():
                ctx.mp2_follow_dev(swap2[turn[1]], n_cifs)
                turn[1] ^= 1

            def both():
                follow_mp2()
                ctx.pad_labels_dev(pswap[turn[2]])
                turn[2] ^= 1

            wall_a, dev_a = timed(follow_plus)
            wall_b, dev_b = timed(follow_mp2)
            wall_c, dev_c = timed(both)
            res = np.stack([o[0].cpu().numpy().view(dabgpu.MP2_RESULT_DTYPE)[0] for o in outs])
            shown = sum(bytes(o[1].cpu().numpy()[16:16 + len(text)]) == text for o in outs)
            in_bytes = sum(3 * br * n_cifs for br in mp2)
            lines += ["%d x %d frames (%d logical frames per entry; the last layer-II call emitted %d rows, %d header errors, %d CRC failures; "
                      "%d of %d entries show the label; %.1f MB of layer-II frames):" %
                      (a.streams, fps, n_cifs, res["frames"].sum(), res["header_errors"].sum(), res["crc_failed"].sum(), shown, len(mp2), in_bytes / 1e6),
                      "  (a) the DAB+ follow call alone        %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_a, dev_a, a.reps),
                      "  (b) the layer-II follow call alone    %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_b, dev_b, a.reps),
                      "  (c) ... and the label call behind it  %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_c, dev_c, a.reps)]
            del keep, swap_plus, swap2, pswap, outs
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mp2_follow_time.txt"))
    ap.add_argument("--limit", type=int, default=600, help="seconds the GPU visit may take")
    ap.add_argument("--commit", default=None, help="what the file says it was measured on (default: git's HEAD)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.commit is None:
        a.commit = commit_name()
    if a.child:
        a.frames = [int(x) for x in a.frames.split(",")]
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--streams", str(a.streams), "--frames", a.frames, "--reps", str(a.reps),
           "--out", a.out, "--commit", a.commit]
    try:
        sys.exit(subprocess.run(cmd, timeout=a.limit).returncode)
    except subprocess.TimeoutExpired:
        sys.exit("mp2_follow_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
