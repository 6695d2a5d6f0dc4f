"""Device time of the reception-quality kernels at the bench's config-4 shape (64 ensembles x 256 frames resident in HBM, the
FIC + one 64 kbit/s EEP-3A sub-channel), timed with device events after warm-up, next to each kernel's byte bound.

  python tools/quality_timing.py [--streams 64] [--frames 256] [--iters 20]

The soft bits and decoded bytes are random (the kernels' work does not depend on the values); one JSON line at the end."""
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
    g.manual_seed(4)
    sc = dabgpu.subchannel(0, 64, level=3)
    soft = torch.randint(-127, 128, (n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev, generator=g)
    fib = torch.randint(0, 256, (n, 12, 32), dtype=torch.uint8, device=dev, generator=g)
    out = torch.randint(0, 256, (n_streams, fps * 4, 192), dtype=torch.uint8, device=dev, generator=g)
    mer = torch.zeros((n, 24), dtype=torch.uint8, device=dev)
    fic_ber = torch.zeros((n, 4, 8), dtype=torch.uint8, device=dev)
    msc_ber = torch.zeros((n_streams, fps * 4, 8), dtype=torch.uint8, device=dev)
    ctx = dabgpu.Context(device=0, max_frames=64)
    s = ctx.stream

    def ber():
        ctx.channel_ber_dev(soft.data_ptr(), dabgpu.NB_FRAME_BITS, n_streams, fps, fib.data_ptr(), fic_ber.data_ptr(), [sc], None,
                            [out.data_ptr()], [msc_ber.data_ptr()], stream=s)

    def ber_fic():
        ctx.channel_ber_dev(soft.data_ptr(), dabgpu.NB_FRAME_BITS, n_streams, fps, fib.data_ptr(), fic_ber.data_ptr(), stream=s)

    def ber_msc():
        ctx.channel_ber_dev(soft.data_ptr(), dabgpu.NB_FRAME_BITS, n_streams, fps, None, None, [sc], None, [out.data_ptr()],
                            [msc_ber.data_ptr()], stream=s)

    def mer_all():
        ctx.mer_dev(soft.data_ptr(), dabgpu.NB_FRAME_BITS, n, mer.data_ptr(), 0, 75, stream=s)

    def mer_fic():
        ctx.mer_dev(soft.data_ptr(), dabgpu.NB_FRAME_BITS, n, mer.data_ptr(), 0, 3, stream=s)

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

    torch.cuda.synchronize()
    # bytes each kernel must read: the punctured soft bits (FIC 9216 + 4 CIFs x 48 CU x 64) and the decoded bytes
    # (4 x 96 FIB bytes + 4 x 192) per frame; the MER kernel its symbols' soft bits
    ber_bytes = n * (9216 + 4 * sc.length * 64 + 4 * 96 + 4 * 192)
    rows = {}
    for name, fn, nbytes in (("channel_ber_fic_plus_msc64", ber, ber_bytes),
                             ("channel_ber_fic_only", ber_fic, n * (9216 + 4 * 96)),
                             ("channel_ber_msc64_only", ber_msc, n * 4 * (sc.length * 64 + 192)),
                             ("mer_all_symbols", mer_all, n * 75 * 3072),
                             ("mer_fic_symbols", mer_fic, n * 3 * 3072)):
        med, mean = timed(fn)
        bound = nbytes / HBM_BPS * 1e3
        rows[name] = {"median_ms": med, "mean_ms": mean, "bytes": nbytes, "bound_ms_at_8TBps": bound, "fraction_of_bound": bound / med}
        print("%-28s median %.4f ms  mean %.4f ms  %.3f GB  bound %.4f ms  fraction %.2f"
              % (name, med, mean, nbytes / 1e9, bound, bound / med))
    ctx.close()
    print(json.dumps({"frames": n, "streams": n_streams, "frames_per_stream": fps, "subchannel": "64 kbit/s EEP-3A", "iters": a.iters,
                      "kernels": rows}))


if __name__ == "__main__":
    main()
