"""Device time of the ETI(NI) launch (dabgpu_eti_frames_dev) for the 18-sub-channel multiplex at the bench's shape
(64 ensembles x 256 frames = 65 536 CIFs, 403 MB of frames), with the library's own events (dabgpu_mean_kernel_ms 7),
beside (a) the decode call it follows (index 2) and (b) plain device-to-device copies, measured in the same run: of the
403 MB it writes, and of those plus the bytes it reads (FIBs + sub-channel bytes).

  python tools/eti_timing.py [--streams 64] [--frames 256] [--iters 20] [--no-decode]

The inputs are random (the work does not depend on the values); one JSON line at the end."""
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


def multiplex18():
    scs, cu = [], 0
    for br, lvl, k in ((64, 3, 10), (48, 3, 4), (32, 2, 3)):
        for _ in range(k):
            x = dabgpu.subchannel(cu, br, level=lvl)
            scs.append(x)
            cu += x.length
    scs.append(dabgpu.uep_subchannel(35, cu))
    return scs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-decode", action="store_true", help="skip the decode call (its soft bits take 3.8 GB)")
    a = ap.parse_args()
    E, F = a.streams, a.frames
    n, n_cif = E * F, F * 4
    dev = torch.device("cuda", 0)
    scs = multiplex18()
    plan = dabgpu.eti_layout([(i, sc) for i, sc in enumerate(scs)])
    u8 = dict(dtype=torch.uint8, device=dev)
    fib = torch.randint(0, 256, (n, 12, 32), **u8)
    ok = torch.ones((n, 12), **u8)
    outs = [torch.randint(0, 256, (E, n_cif, sc.bitrate_kbps * 3), **u8) for sc in scs]
    eti = torch.empty((E, n_cif, dabgpu.ETI_FRAME_BYTES), **u8)
    status = torch.empty((E, n_cif, 8), **u8)
    hist = [torch.zeros((E, dabgpu.eti_history_bytes()), **u8) for _ in range(2)]
    ctx = dabgpu.Context(device=0, max_frames=n)
    s = ctx.stream
    ext = torch.cuda.ExternalStream(s)
    torch.cuda.synchronize()

    def eti_call():
        ctx.eti_frames_dev(plan, E, F, fib.data_ptr(), ok.data_ptr(), [o.data_ptr() for o in outs], eti.data_ptr(),
                           status.data_ptr(), d_history_in=hist[0].data_ptr(), d_history_out=hist[1].data_ptr(), stream=s)

    def library_ms(fn, which):
        for _ in range(a.warmup):
            fn()
        ctx.sync()
        ctx.set_timing(True)
        for _ in range(a.iters):
            fn()
        ms, launches = ctx.mean_kernel_ms(which)
        ctx.set_timing(False)
        return ms, launches

    def copy_ms(dst, src):
        with torch.cuda.stream(ext):
            for _ in range(a.warmup):
                dst.copy_(src)
            ms = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ext)
                dst.copy_(src)
                e1.record(ext)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        ms.sort()
        return ms[len(ms) // 2]

    eti_ms, launches = library_ms(eti_call, 7)
    written = eti.numel() + status.numel() + hist[1].numel()
    read = fib.numel() + ok.numel() + sum(o.numel() for o in outs)
    src = torch.empty(written + read, **u8)
    dst = torch.empty(written + read, **u8)
    torch.cuda.synchronize()
    copy_out_ms = copy_ms(dst[:written], src[:written])
    copy_all_ms = copy_ms(dst[:(written + read) // 2], src[:(written + read) // 2])   # moves read + written bytes in all
    del src, dst
    row = {"frames": n, "cifs": E * n_cif, "eti_ms": eti_ms, "eti_launches_timed": launches, "bytes_written": written,
           "bytes_read": read, "copy_of_the_written_bytes_ms": copy_out_ms, "copy_moving_read_plus_written_bytes_ms": copy_all_ms,
           "eti_over_copy_of_written": eti_ms / copy_out_ms, "eti_over_copy_of_same_traffic": eti_ms / copy_all_ms,
           "eti_GBps": (written + read) / eti_ms / 1e6}
    print("ETI launch (anchor + frames), %d CIFs: mean %.4f ms over %d launches; %.1f MB written, %.1f MB read: %.0f GB/s"
          % (E * n_cif, eti_ms, launches, written / 1e6, read / 1e6, row["eti_GBps"]))
    print("device-to-device copy of the %.1f MB written: median %.4f ms  -> ETI / copy = %.2f" % (written / 1e6, copy_out_ms, row["eti_over_copy_of_written"]))
    print("device-to-device copy with the same traffic (%.1f MB read + written in all): median %.4f ms  -> ETI / copy = %.2f"
          % ((written + read) / 1e6, copy_all_ms, row["eti_over_copy_of_same_traffic"]))
    if not a.no_decode:
        torch.cuda.empty_cache()
        soft = torch.randint(-127, 128, (n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
        torch.cuda.synchronize()
        dec_ms, _ = library_ms(lambda: ctx.decode_frames_dev(soft.data_ptr(), dabgpu.NB_FRAME_BITS, E, F, fib.data_ptr(), ok.data_ptr(),
                                                             scs, None, None, [o.data_ptr() for o in outs], s), 2)
        row.update(decode_ms=dec_ms, eti_over_decode=eti_ms / dec_ms)
        print("the decode call it follows (FIC + 18 sub-channels): mean %.3f ms  -> ETI / decode = %.3f" % (dec_ms, eti_ms / dec_ms))
    ctx.close()
    print(json.dumps(row))


if __name__ == "__main__":
    main()
