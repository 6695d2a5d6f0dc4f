#!/usr/bin/env python3
"""Time dabgpu_decode_ensembles_dev on a batch of ensembles that each have their own multiplex (GPU box).

  python tools/ensembles_time.py [--streams 64] [--frames 16,256] [--reps 20] [--out profiles/ensembles_time.txt] [--limit 600]

One visit to the GPU, in a child process that is ended after --limit seconds.  A fixed seed gives every stream 6-18
sub-channels of mixed EEP-A, EEP-B and UEP profiles (start addresses, sizes and number differ from stream to stream); the
soft bits are noise (the decoder's time does not depend on the data).  Per batch shape the child times, as stream-synchronised
wall time over --reps repetitions after two warm-up calls (so that what the host spends on launches counts):
  (a) the ragged call: dabgpu_decode_ensembles_dev, every stream its own plan
  (b) what a caller has without it: one dabgpu_decode_frames_dev per stream (n_streams = 1) on the same buffers
  (c) every stream given the SAME plan: the ragged call (entry table in device memory) against the single
      dabgpu_decode_frames_dev call (entry table by value, 16 entries a launch)
and reads the library's own events for the parts of (a) (forward pass | traceback | history rings)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def random_plan(dabgpu, rng):
    """6-18 sub-channels from a random first capacity unit, with random gaps between them"""
    kinds = [("eep", 0, 3, 64), ("eep", 0, 3, 48), ("eep", 0, 2, 32), ("eep", 0, 4, 96), ("eep", 0, 1, 16), ("eep", 0, 3, 8),
             ("eep", 1, 3, 32), ("eep", 1, 2, 64), ("eep", 1, 4, 96), ("uep", 17), ("uep", 4), ("uep", 35), ("uep", 15), ("uep", 0)]
    small = ("eep", 0, 3, 8)                                    # 6 CU: what a nearly full CIF still holds

    def size(k):
        return dabgpu.uep_subchannel(k[1], 0).length if k[0] == "uep" else dabgpu.subchannel(0, k[3], level=k[2], eep_type=k[1]).length

    want = int(rng.integers(6, 19))
    scs, cu = [], int(rng.integers(0, 8))
    while len(scs) < want:
        k = kinds[int(rng.integers(0, len(kinds)))]
        if cu + size(k) > 864:
            k = small
        if cu + size(k) > 864:
            break
        scs.append(dabgpu.uep_subchannel(k[1], cu) if k[0] == "uep" else dabgpu.subchannel(cu, k[3], level=k[2], eep_type=k[1]))
        cu += scs[-1].length + int(rng.integers(0, 3))
    return scs


def child(a):
    import numpy as np
    import torch
    import dabgpu
    dev = torch.device("cuda", 0)
    FB = dabgpu.NB_FRAME_BITS
    rng = np.random.default_rng(2024)
    plans = [random_plan(dabgpu, rng) for _ in range(a.streams)]
    lines = ["ensembles_time: %d ensembles, %d..%d sub-channels each (%d entries, %d kbit/s in all), %s" %
             (a.streams, min(map(len, plans)), max(map(len, plans)), sum(map(len, plans)),
              sum(sc.bitrate_kbps for p in plans for sc in p), torch.cuda.get_device_name(0))]

    def timed(ctx, run):
        for _ in range(2):
            run()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            run()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / a.reps

    for fps in a.frames:
        n = a.streams * fps
        soft = torch.empty((n, FB), dtype=torch.int8, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(fps)
        for f0 in range(0, n, 1024):
            soft[f0:f0 + 1024] = torch.randint(-127, 128, (min(1024, n - f0), FB), dtype=torch.int8, device=dev, generator=g)
        fib = torch.zeros((n, 12, 32), dtype=torch.uint8, device=dev)
        ok = torch.zeros((n, 12), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def own(plans_):
            outs = [[torch.zeros((fps * 4, sc.bitrate_kbps * 3), dtype=torch.uint8, device=dev) for sc in p] for p in plans_]
            hout = [[torch.zeros((15, sc.length * 64), dtype=torch.int8, device=dev) for sc in p] for p in plans_]
            return outs, hout, [[o.data_ptr() for o in lst] for lst in outs], [[h.data_ptr() for h in lst] for lst in hout]

        with dabgpu.Context(device=0, max_frames=64) as ctx:
            outs, hout, p_out, p_hout = own(plans)
            torch.cuda.synchronize()
            ragged = lambda: ctx.decode_ensembles_dev(soft.data_ptr(), FB, a.streams, fps, fib.data_ptr(), ok.data_ptr(), plans, None,
                                                      p_hout, p_out)
            def one_by_one():
                for s in range(a.streams):
                    ctx.decode_frames_dev(soft.data_ptr() + s * fps * FB, FB, 1, fps, fib.data_ptr() + s * fps * 384,
                                          ok.data_ptr() + s * fps * 12, plans[s], None, p_hout[s], p_out[s])
            ms_a = timed(ctx, ragged)
            ctx.set_timing(True)
            for _ in range(3):
                ragged()
            ctx.sync()
            whole = ctx.mean_kernel_ms(2)[0]
            try:
                parts = [ctx.mean_kernel_ms(w)[0] for w in (4, 5, 6)]
            except dabgpu.DabGpuError:
                parts = None                                    # (the call went part by part: no grouped launch to split)
            ctx.set_timing(False)
            ms_b = timed(ctx, one_by_one)
            del outs, hout
            # (c) the same plan for everybody
            same = [plans[0]] * a.streams
            outs, hout, p_out, p_hout = own(same)
            u_out = [torch.zeros((a.streams, fps * 4, sc.bitrate_kbps * 3), dtype=torch.uint8, device=dev) for sc in plans[0]]
            u_hout = [torch.zeros((a.streams, 15, sc.length * 64), dtype=torch.int8, device=dev) for sc in plans[0]]
            torch.cuda.synchronize()
            ms_c_ragged = timed(ctx, lambda: ctx.decode_ensembles_dev(soft.data_ptr(), FB, a.streams, fps, fib.data_ptr(), ok.data_ptr(),
                                                                      same, None, p_hout, p_out))
            ms_c_single = timed(ctx, lambda: ctx.decode_frames_dev(soft.data_ptr(), FB, a.streams, fps, fib.data_ptr(), ok.data_ptr(), plans[0],
                                                                   None, [h.data_ptr() for h in u_hout], [o.data_ptr() for o in u_out]))
            del outs, hout, u_out, u_hout
        lines += ["%d x %d frames (%d codewords of the FIC, %d of sub-channels):" % (a.streams, fps, 4 * n, 4 * fps * sum(map(len, plans))),
                  "  (a) ragged call, own plans            %9.3f ms  (mean of %d, wall)" % (ms_a, a.reps),
                  "      its device time                   %9.3f ms  %s" %
                  (whole, "forward %.3f | traceback %.3f | history rings %.3f" % tuple(parts) if parts else "(part by part)"),
                  "  (b) one call per stream, own plans    %9.3f ms  (mean of %d, wall)   (b) / (a) = %.2f" % (ms_b, a.reps, ms_b / ms_a),
                  "  (c) one plan of %2d for every stream:  ragged %9.3f ms, single dabgpu_decode_frames_dev %9.3f ms   ragged / single = %.3f" %
                  (len(plans[0]), ms_c_ragged, ms_c_single, ms_c_ragged / ms_c_single)]
        del soft, fib, ok
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensembles_time.txt"))
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
        sys.exit("ensembles_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
