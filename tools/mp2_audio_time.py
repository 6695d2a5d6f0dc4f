#!/usr/bin/env python3
"""Time dabgpu_mp2_subbands_dev behind dabgpu_mp2_follow_dev on the layer-II entries of a batch of ensembles (GPU box).

  python tools/mp2_audio_time.py [--streams 64] [--frames 16,256] [--reps 20] [--out profiles/mp2_audio_time.txt] [--limit 900]
                                 [--commit <what the file says it was measured on>]

One visit to the GPU, in a child process that is ended after --limit seconds.  The plans are those of
tools/mp2_follow_time.py (same seed): their UEP sub-channels are the layer-II entries.  Every entry repeats a cycle of 20
frames at 48 kHz with the ISO CRC and a whole audio part (synth.mp2_audio_frame: random allocation, SCFSI, scale factors and
samples, lowered until they fit).  Per batch shape the child times, over --reps repetitions after two warm-up calls, as
stream-synchronised wall time and between two events on the stream:
  (a) the follow call alone, the carry records swapped between calls
  (b) the follow call and the level call behind it on the same stream, d_subbands NULL
  (c) the same with d_subbands given
and, once, the host twin dabgpu_mp2_subbands_host on the same table in host memory (levels only), with the bytes the level
call reads and writes.  No time is fixed in advance: the file records what was measured, and on what."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mp2_follow_time import commit_name  # noqa: E402


def child(a):
    import numpy as np
    import torch
    import dabgpu
    from dabgpu import synth
    from ensembles_time import random_plan
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2024)
    plans = [random_plan(dabgpu, rng) for _ in range(a.streams)]
    mp2 = [sc.bitrate_kbps for p in plans for sc in p if sc.is_uep]
    lines = ["mp2_audio_time: measured on %s, %s" % (a.commit, torch.cuda.get_device_name(0)),
             "%d ensembles: %d layer-II entries (%d kbit/s in all, %d..%d each)" % (a.streams, len(mp2), sum(mp2), min(mp2), max(mp2))]
    cycle = {}
    for br in sorted(set(mp2)):
        mode = synth.MP2_MONO if br in (32, 48, 56, 80) else synth.MP2_STEREO
        cycle[br] = np.stack([synth.mp2_audio_frame(rng, br, mode=mode)[0] for _k in range(20)])
    zeros = lambda n: torch.zeros((n,), dtype=torch.uint8, device=dev)
    values = 4 * 2 * 36 * 32

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
            keep, swap, levels_only, with_values, outs, host = [], [[], []], [[], []], [[], []], [], []
            for e, br in enumerate(mp2):
                frames_h = np.ascontiguousarray(cycle[br][(np.arange(n_cifs) - e % 7) % 20])
                frames = torch.from_numpy(frames_h).to(dev)
                rows, st, fo, res = zeros((n_cifs + 1) * 220), zeros((n_cifs + 1) * 64), zeros(32), zeros(64)
                c0, c1 = zeros(dabgpu.mp2_carry_bytes(br)), zeros(dabgpu.mp2_carry_bytes(br))
                lev, sub, aud = zeros((n_cifs + 1) * 32), zeros((n_cifs + 1) * values), zeros(32)
                keep += [frames, rows, st, fo, c0, c1, sub]
                outs.append((res, lev, aud))
                host.append(frames_h)
                for side, (ci, co) in enumerate(((c0, c1), (c1, c0))):
                    swap[side].append(dabgpu.Mp2Entry(frames.data_ptr(), 3 * br, br, ci.data_ptr(), co.data_ptr(), rows.data_ptr(), st.data_ptr(),
                                                      fo.data_ptr(), res.data_ptr()))
                    for table, d_sub in ((levels_only, None), (with_values, sub.data_ptr())):
                        table[side].append(dabgpu.Mp2AudioEntry(frames.data_ptr(), 3 * br, br, ci.data_ptr(), st.data_ptr(), res.data_ptr(),
                                                                lev.data_ptr(), d_sub, aud.data_ptr()))
            torch.cuda.synchronize()
            turn = [0]

            def follow(table=None):
                ctx.mp2_follow_dev(swap[turn[0]], n_cifs)
                if table is not None:
                    ctx.mp2_subbands_dev(table[turn[0]], n_cifs)
                turn[0] ^= 1

            wall_a, dev_a = timed(follow)
            wall_b, dev_b = timed(lambda: follow(levels_only))
            wall_c, dev_c = timed(lambda: follow(with_values))
            aud = np.stack([o[2].cpu().numpy().view(dabgpu.MP2_AUDIO_RESULT_DTYPE)[0] for o in outs])
            lev = np.concatenate([o[1].cpu().numpy().view(dabgpu.MP2_LEVEL_DTYPE)[:n_cifs] for o in outs])
            # the host twin, once, on the same frames in host memory: the follow twin first (untimed), then the level call
            hk, f_entries, a_entries = [], [], []
            for br, frames_h in zip(mp2, host):
                bufs = [np.zeros(n, np.uint8) for n in (dabgpu.mp2_carry_bytes(br) + 16, (n_cifs + 1) * 220, (n_cifs + 1) * 64, 32, 64,
                                                         (n_cifs + 1) * 32, 32)]
                hk += bufs + [frames_h]
                co = bufs[0].ctypes.data + (-bufs[0].ctypes.data) % 16
                p = [b.ctypes.data for b in bufs]
                f_entries.append(dabgpu.Mp2Entry(frames_h.ctypes.data, 3 * br, br, None, co, p[1], p[2], p[3], p[4]))
                a_entries.append(dabgpu.Mp2AudioEntry(frames_h.ctypes.data, 3 * br, br, None, p[2], p[4], p[5], None, p[6]))
            dabgpu.mp2_follow_host(f_entries, n_cifs)
            t0 = time.perf_counter()
            dabgpu.mp2_subbands_host(a_entries, n_cifs)
            host_ms = (time.perf_counter() - t0) * 1e3
            in_bytes = sum(3 * br * n_cifs for br in mp2)
            out_levels, out_values = len(mp2) * n_cifs * 32, len(mp2) * n_cifs * values
            lines += ["%d x %d frames (%d logical frames per entry; the last level call decoded %d frames, %d not good, %d overrun, %d silent; "
                      "mean power per decoded frame %.3g):" %
                      (a.streams, fps, n_cifs, aud["decoded"].sum(), aud["not_good"].sum(), aud["overrun"].sum(), aud["silent"].sum(),
                       float(lev["power"].sum()) / max(1, int(aud["decoded"].sum()))),
                      "  (a) the follow call alone                  %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_a, dev_a, a.reps),
                      "  (b) ... and the level call behind it       %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_b, dev_b, a.reps),
                      "  (c) ... with the sub-band samples written  %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_c, dev_c, a.reps),
                      "  the level call reads %.1f MB of frames and writes %.2f MB of level records, with sub-bands %.1f MB more" %
                      (in_bytes / 1e6, out_levels / 1e6, out_values / 1e6),
                      "  the host twin, levels only, one thread     %9.1f ms  (once)" % host_ms]
            del keep, swap, levels_only, with_values, outs, host, hk
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mp2_audio_time.txt"))
    ap.add_argument("--limit", type=int, default=900, help="seconds the GPU visit may take")
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
        sys.exit("mp2_audio_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
