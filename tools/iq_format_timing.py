"""Front end and host-fed ring on each sample format (dabgpu_set_iq_format): cf32, cs16, cs8, cu8.

  python tools/iq_format_timing.py [--streams 64] [--frames 256] [--iters 12] [--ring-batches 24]

Front end: the bench's shape (64 streams x 256 frames resident in HBM, frame_stride 196608, closed loop), all soft bits and
then FIC + one 64 kbit/s sub-channel; one context per format, launches alternated between the formats inside this process and
timed with the library's events (dabgpu_mean_kernel_ms(ctx, 0)).  TB/s on each format's algorithmic bytes per frame
(samples read + soft bits written: 1 782 016 / 1 006 208 / 618 304 B for cf32 / cs16 / cs8+cu8).  The soft bits of every
integer format are hashed against the cf32 path's on a float32 copy of the same values.
Ring: frames/s per format, 64 frames per submit, 3 slots, FIC + the sub-channel decoded, buffers from dabgpu_host_alloc.
The samples are noise (the front end's work does not depend on their values).  One JSON line at the end."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dabgpu  # noqa: E402

HBM_BPS = 8e12
SYMS = 76 * 2552
FMTS = {"cf32": dabgpu.IQ_CF32, "cs16": dabgpu.IQ_CS16, "cs8": dabgpu.IQ_CS8, "cu8": dabgpu.IQ_CU8}
SAMPLE_BYTES = {"cf32": 8, "cs16": 4, "cs8": 2, "cu8": 2}


def frame_bytes(fmt):
    # samples the fused kernel reads per frame (76 whole symbols, prefixes included) + the soft bits it writes
    return SYMS * SAMPLE_BYTES[fmt] + dabgpu.NB_FRAME_BITS


def as_cf32(t, fmt):
    """float32 copy [n, stride, 2] of integer samples: the values the kernels work on"""
    v = t.to(torch.float32)
    return v.sub_(127.5) if fmt == "cu8" else v


def selection():
    sc = dabgpu.subchannel(0, 64, level=3)
    return sc, [(0, 9216)] + [(9216 + c * 55296 + sc.start_address * 64, sc.length * 64) for c in range(4)]


def front_end(a, dev):
    S, F = a.streams, a.frames
    n, stride = S * F, dabgpu.NB_FRAME_SAMPLES
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    bufs = {"cs16": torch.randint(-3000, 3001, (n, stride, 2), dtype=torch.int16, device=dev, generator=g),
            "cs8": torch.randint(-40, 41, (n, stride, 2), dtype=torch.int8, device=dev, generator=g),
            "cu8": torch.randint(87, 169, (n, stride, 2), dtype=torch.uint8, device=dev, generator=g)}
    bufs["cf32"] = as_cf32(bufs["cs16"], "cs16")
    soft = {k: torch.empty((n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev) for k in FMTS}
    ctxs = {}
    for k, f in FMTS.items():
        c = dabgpu.Context(device=0, max_frames=64)
        c.set_iq_format(f)
        ctxs[k] = c
    _, ranges = selection()
    out = {"shape": {"streams": S, "frames": F, "frame_stride": stride}, "front_end": {}, "hash_equal": {}}

    def launch(k, iq=None):
        c = ctxs[k]
        c.ofdm_demod_streams_dev((iq if iq is not None else bufs[k]).data_ptr(), stride, S, F, 0.9, soft[k].data_ptr())

    # bit-exactness at this size: each integer format against cf32 on a float32 copy of its values
    for sel in (None, ranges):
        for k in ("cs16", "cs8", "cu8"):
            ref = as_cf32(bufs[k], k) if k != "cs16" else bufs["cf32"]
            for c in ctxs.values():
                c.set_soft_selection(sel)
            ctxs["cf32"].streams_reset(S)
            ctxs[k].streams_reset(S)
            soft["cf32"].fill_(0)
            soft[k].fill_(0)
            torch.cuda.synchronize()                            # (the library's stream is not ordered behind torch's)
            launch("cf32", ref)
            launch(k)
            torch.cuda.synchronize()
            h = [hashlib.sha256(soft[x].cpu().numpy().tobytes()).hexdigest()[:16] for x in ("cf32", k)]
            out["hash_equal"]["%s%s" % (k, "+sel" if sel else "")] = h[0] == h[1]
            print("hash %-4s %s: cf32-of-same-values %s, %s %s" % (k, "FIC+64k" if sel else "all", h[0], k, h[1]), flush=True)
            del ref
        torch.cuda.empty_cache()
    # timing, formats alternated launch by launch
    torch.cuda.synchronize()
    for sel_name, sel in (("all", None), ("fic+64k", ranges)):
        for c in ctxs.values():
            c.set_soft_selection(sel)
            c.streams_reset(S)
            c.set_timing(False)
        for _ in range(a.warmup):
            for k in FMTS:
                launch(k)
                torch.cuda.synchronize()
        for c in ctxs.values():
            c.set_timing(True)
        for _ in range(a.iters):
            for k in FMTS:
                launch(k)
                torch.cuda.synchronize()                        # one launch on the device at a time (four streams)
        res = {}
        for k, c in ctxs.items():
            ms, cnt = c.mean_kernel_ms(0)
            tbps = n * frame_bytes(k) / (ms * 1e-3) / 1e12
            res[k] = {"ms": round(ms, 3), "launches": cnt, "frames_per_s": round(n / (ms * 1e-3)), "bytes_per_frame": frame_bytes(k),
                      "tb_per_s": round(tbps, 2), "hbm_fraction": round(tbps * 1e12 / HBM_BPS, 3)}
            print("front end %-8s %-4s %8.3f ms  %9.0f frames/s  %5.2f TB/s on %d B/frame" % (sel_name, k, ms, n / (ms * 1e-3), tbps,
                                                                                            frame_bytes(k)), flush=True)
        out["front_end"][sel_name] = res
    for c in ctxs.values():
        c.close()
    del bufs, soft
    torch.cuda.empty_cache()
    return out


def ring(a):
    batch, slots = 64, 3
    sc, _ = selection()
    rng = np.random.default_rng(3)
    res = {}
    for k in ("cs16", "cs8", "cu8", "cf32"):
        c = dabgpu.Context(device=0, max_frames=64)
        c.set_iq_format(FMTS[k])
        if k == "cf32":
            iq = dabgpu.PinnedArray((batch, SYMS), np.complex64)
            iq.array.view(np.float32)[:] = rng.integers(-3000, 3001, size=(batch, 2 * SYMS)).astype(np.float32)
        else:
            dt = {"cs16": np.int16, "cs8": np.int8, "cu8": np.uint8}[k]
            iq = dabgpu.PinnedArray((batch, SYMS, 2), dt)
            lo, hi = {"cs16": (-3000, 3001), "cs8": (-40, 41), "cu8": (87, 169)}[k]
            iq.array[:] = rng.integers(lo, hi, size=(batch, SYMS, 2)).astype(dt)
        fo = dabgpu.PinnedArray((batch,), np.float32)
        fo.array[:] = 0.0
        fib = [dabgpu.PinnedArray((batch, 12, 32), np.uint8) for _ in range(slots)]
        ok = [dabgpu.PinnedArray((batch, 12), np.uint8) for _ in range(slots)]
        msc = [dabgpu.PinnedArray((batch * 4, 192), np.uint8) for _ in range(slots)]
        c.pipe_open(slots, batch, SYMS)
        t0 = None
        tickets = []
        for b in range(a.ring_batches + 6):
            if b == 6:                                          # six batches of warm-up
                for t in tickets:
                    c.pipe_wait(t)
                tickets = []
                t0 = time.perf_counter()
            j = b % slots
            tickets.append(c.pipe_submit(iq.array, 1, batch, fo.array, [sc], None, fib[j].array, ok[j].array, [msc[j].array]))
        for t in tickets:
            c.pipe_wait(t)
        dt_s = time.perf_counter() - t0
        fps = a.ring_batches * batch / dt_s
        up = fps * SYMS * SAMPLE_BYTES[k]
        res[k] = {"frames_per_s": round(fps), "upload_GB_per_s": round(up / 1e9, 2)}
        print("ring %-4s %8.0f frames/s  (%.1f GB/s of samples up)" % (k, fps, up / 1e9), flush=True)
        c.pipe_close()
        c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ring-batches", type=int, default=24)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = front_end(a, dev)
    out["ring"] = ring(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
