"""Device time of the channel impulse response (dabgpu_cir_frames_dev) at the bench's shape (64 ensembles x 256 frames =
16 384 frames), timed with device events after warm-up, next to its byte bound.  Two layouts: whole frames at the front
end's stride (196 608 samples: each frame's 16 KB window read out of a 25.8 GB buffer) and PRS symbols packed at 2552
samples.

  python tools/cir_timing.py [--streams 64] [--frames 256] [--iters 20]

The samples are random (the kernels' work does not depend on the values); one JSON line at the end."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import dabgpu  # noqa: E402

HBM_BPS = 8e12
SYM = 2552
REC = dabgpu.CIR_ACC_DTYPE.itemsize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n_streams, fps = a.streams, a.frames
    n = n_streams * fps
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    fo = (torch.rand(n, device=dev, generator=g) - 0.5) / 2048
    acc = torch.zeros((n_streams, REC), dtype=torch.uint8, device=dev)
    frame = torch.zeros((n, REC), dtype=torch.uint8, device=dev)
    ctx = dabgpu.Context(device=0, max_frames=64)
    ctx.streams_reset(n_streams)
    s = ctx.stream

    def timed(fn):
        ext = torch.cuda.ExternalStream(s)
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext)
            fn()
            e1.record(ext)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        return ms[len(ms) // 2], sum(ms) / len(ms)

    rows = {}
    nbytes = n * 2048 * 8 + n * REC * 2 + n_streams * REC * 2          # windows, records out and back, accumulators
    for layout, stride in (("bench_stride", dabgpu.NB_FRAME_SAMPLES), ("packed_prs", SYM)):
        iq = torch.randn((n * stride + SYM) * 2, device=dev, generator=g)
        torch.cuda.synchronize()
        base = iq.data_ptr()
        cases = (("%s_freq_array" % layout, lambda: ctx.cir_frames_dev(base, stride, n_streams, fps, acc.data_ptr(),
                                                                      d_freq_offset=fo.data_ptr(), stream=s)),
                 ("%s_states" % layout, lambda: ctx.cir_frames_dev(base, stride, n_streams, fps, acc.data_ptr(), stream=s)),
                 ("%s_with_frame_records" % layout, lambda: ctx.cir_frames_dev(base, stride, n_streams, fps, acc.data_ptr(),
                                                                             d_freq_offset=fo.data_ptr(), d_frame=frame.data_ptr(),
                                                                             stream=s)))
        for name, fn in cases:
            med, mean = timed(fn)
            bound = nbytes / HBM_BPS * 1e3
            rows[name] = {"median_ms": med, "mean_ms": mean, "bytes": nbytes, "bound_ms_at_8TBps": bound, "fraction_of_bound": bound / med}
            print("%-36s median %.4f ms  mean %.4f ms  %.3f GB  bound %.4f ms  fraction %.2f"
                  % (name, med, mean, nbytes / 1e9, bound, bound / med))
        del iq
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"frames": n, "streams": n_streams, "frames_per_stream": fps, "iters": a.iters, "kernels": rows}))


if __name__ == "__main__":
    main()
