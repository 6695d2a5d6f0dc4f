#!/usr/bin/env python3
"""Time dabgpu_dabplus_follow_dev on the DAB+ entries of a batch of ensembles (GPU box).

  python tools/dabplus_follow_time.py [--streams 64] [--frames 16,256] [--reps 20] [--out profiles/dabplus_follow_time.txt] [--limit 600]

One visit to the GPU, in a child process that is ended after --limit seconds.  The plans are those of
tools/ensembles_time.py (same seed: 6-18 sub-channels per stream); their EEP entries are taken as the DAB+ ones.  Every
entry's logical frames are device-resident, as the decode call leaves them: super-frames of dabgpu.synth one after the
other from an offset of the entry's own.  Per batch shape the child times, over --reps repetitions after two warm-up calls,
as stream-synchronised wall time (what the host spends on launches counts) and between two events on the stream:
  (a) one follow call for all entries, the carry records swapped between calls
  (b) what a caller had without it: one dabgpu_dabplus_superframes_dev call per entry on the same frames, the alignment
      TOLD by the host (no search, no carry: this favours (b))."""
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
    lines = ["dabplus_follow_time: %d ensembles, %d DAB+ entries (%d kbit/s in all, %d..%d each), %s" %
             (a.streams, len(rates), sum(rates), min(rates), max(rates), torch.cuda.get_device_name(0))]
    cycle = {br: np.concatenate([synth.build_superframe(rng, br, 1, 1)[0] for _ in range(4)]).reshape(20, 3 * br) for br in sorted(set(rates))}

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
            keep, swap, aligned = [], [[], []], []
            n_sf_b = 0
            for e, br in enumerate(rates):
                s, off = br // 8, e % 5
                frames = torch.from_numpy(np.ascontiguousarray(cycle[br][(np.arange(n_cifs) - off) % 20])).to(dev)
                data = torch.zeros((max_sf, 110 * s), dtype=torch.uint8, device=dev)
                st = torch.zeros((max_sf * 64,), dtype=torch.uint8, device=dev)
                res = torch.zeros((32,), dtype=torch.uint8, device=dev)
                c0, c1 = (torch.zeros((dabgpu.dabplus_carry_bytes(br),), dtype=torch.uint8, device=dev) for _ in range(2))
                keep += [frames, data, st, res, c0, c1]
                for side, (ci, co) in enumerate(((c0, c1), (c1, c0))):
                    swap[side].append(dabgpu.DabplusEntry(frames.data_ptr(), 3 * br, br, ci.data_ptr(), co.data_ptr(), data.data_ptr(),
                                                          st.data_ptr(), res.data_ptr()))
                n = (n_cifs - off) // 5
                n_sf_b += n
                aligned.append((frames.data_ptr() + off * 3 * br, 15 * br, n, br, data.data_ptr(), st.data_ptr()))
            torch.cuda.synchronize()
            turn = [0]

            def follow():
                ctx.dabplus_follow_dev(swap[turn[0]], n_cifs)
                turn[0] ^= 1

            def one_by_one():
                for d_in, stride, n, br, d_out, d_st in aligned:
                    ctx.dabplus_superframes_dev(d_in, stride, n, br, d_out, d_st)

            wall_a, dev_a = timed(follow)
            got = sum(int(keep[6 * e + 3].cpu().numpy().view(dabgpu.DABPLUS_FOLLOW_RESULT_DTYPE)[0]["n_superframes"]) for e in range(len(rates)))
            wall_b, dev_b = timed(one_by_one)
            lines += ["%d x %d frames (%d logical frames per entry; %d super-frames by (a)'s last call, %d by (b)):" % (a.streams, fps, n_cifs, got, n_sf_b),
                      "  (a) one follow call                   %9.3f ms wall  %9.3f ms between events  (mean of %d)" % (wall_a, dev_a, a.reps),
                      "  (b) one call per entry, aligned by host %7.3f ms wall  %9.3f ms between events  (mean of %d)   (b) / (a) = %.2f wall, %.2f events"
                      % (wall_b, dev_b, a.reps, wall_b / wall_a, dev_b / dev_a)]
            del keep, swap, aligned
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dabplus_follow_time.txt"))
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
        sys.exit("dabplus_follow_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
