#!/usr/bin/env python3
"""Time the modulator's kernels against a plain fill of the same IQ buffer (GPU box).

  python tools/modulator_time.py [--streams 64] [--frames 256] [--out profiles/modulator_time.txt] [--limit 300]

One visit to the GPU, in a child process that is ended after --limit seconds.  The child modulates --streams ensembles x
--frames transmission frames (the bench's batch) of the 18-sub-channel multiplex three times with the library's timers on,
reads the encoder (with its pre-pass) and the symbol kernel through dabgpu_mean_kernel_ms 8 / 9, times a device fill of
the same IQ buffer in the same process -- the write-only ceiling of that box -- and writes both, their ratio and the bytes
moved per frame to --out."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def multiplex18(dabgpu):
    scs, cu = [], 0
    for br, lvl, k in ((64, 3, 10), (48, 3, 4), (32, 2, 3)):
        for _ in range(k):
            x = dabgpu.subchannel(cu, br, level=lvl)
            scs.append(x)
            cu += x.length
    scs.append(dabgpu.uep_subchannel(35, cu))
    return [(i, sc) for i, sc in enumerate(scs)]


def child(a):
    import numpy as np
    import torch
    import dabgpu
    streams = multiplex18(dabgpu)
    plan = dabgpu.eti_layout(streams)
    n_frames, n_cif = a.streams * a.frames, 4 * a.frames
    # 64 different random ETI frames with the plan's header, repeated: the CRCs are not read on the device
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (64, dabgpu.ETI_FRAME_BYTES), dtype=np.uint8)
    base[:, :plan.header_bytes] = np.frombuffer(bytes(plan.header[:plan.header_bytes]), np.uint8)
    base[:, 1:4] = (0x07, 0x3A, 0xB6)
    dev = torch.device("cuda", 0)
    eti = torch.from_numpy(base).to(dev).repeat((a.streams * n_cif + 63) // 64, 1)[:a.streams * n_cif].contiguous()
    iq = torch.empty((n_frames, dabgpu.NB_FRAME_SAMPLES), dtype=torch.complex64, device=dev)
    status = torch.empty((n_frames, 8), dtype=torch.uint8, device=dev)
    state = torch.empty((a.streams, dabgpu.mod_state_bytes()), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with dabgpu.Context(device=0, max_frames=64) as ctx:
        run = lambda: ctx.modulate_eti_dev(plan, streams, a.streams, a.frames, eti.data_ptr(), iq.data_ptr(), status.data_ptr(),
                                           d_state_out=state.data_ptr())
        run()
        ctx.sync()
        ctx.set_timing(True)
        for _ in range(3):
            run()
        ctx.sync()
        enc_ms, n_enc = ctx.mean_kernel_ms(dabgpu.WHICH_MOD_ENCODE)
        sym_ms, n_sym = ctx.mean_kernel_ms(dabgpu.WHICH_MOD_SYMBOLS)
        ctx.set_timing(False)
        refused = int(status.view(torch.int64).ne(0).sum().item())
    flat = torch.view_as_real(iq)
    flat.fill_(0.5)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        flat.fill_(0.25)
    e1.record()
    torch.cuda.synchronize()
    fill_ms = e0.elapsed_time(e1) / 3
    iq_bytes = dabgpu.NB_FRAME_SAMPLES * 8
    coded = 4 * 7200                                            # four coded records
    cum = 75 * 96 * 4                                           # running quarter turns of the 75 data symbols
    lines = ["modulator_time: %d ensembles x %d frames = %d transmission frames, 18 sub-channels (856 CUs), %s" %
             (a.streams, a.frames, n_frames, torch.cuda.get_device_name(0)),
             "bytes per frame: IQ written %d; ETI read %d; coded records written %d (read up to 16 x by the pre-pass, from L2); "
             "running phases written and read %d" % (iq_bytes, 4 * plan.length, coded, cum),
             "encoder + pre-pass   %8.3f ms  (mean of %d)   %6.2f us / frame" % (enc_ms, n_enc, enc_ms * 1e3 / n_frames),
             "symbol kernel        %8.3f ms  (mean of %d)   %6.2f us / frame   %7.1f GB/s of IQ" %
             (sym_ms, n_sym, sym_ms * 1e3 / n_frames, n_frames * iq_bytes / sym_ms / 1e6),
             "fill of the buffer   %8.3f ms  (mean of 3)    %6.2f us / frame   %7.1f GB/s" %
             (fill_ms, fill_ms * 1e3 / n_frames, n_frames * iq_bytes / fill_ms / 1e6),
             "symbol kernel / fill %8.3f      (encoder + pre-pass + symbol kernel) / fill %8.3f" %
             (sym_ms / fill_ms, (enc_ms + sym_ms) / fill_ms),
             "frames with a status other than 0: %d" % refused]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modulator_time.txt"))
    ap.add_argument("--limit", type=int, default=300, help="seconds the GPU visit may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--streams", str(a.streams), "--frames", str(a.frames), "--out", a.out]
    try:
        sys.exit(subprocess.run(cmd, timeout=a.limit).returncode)
    except subprocess.TimeoutExpired:
        sys.exit("modulator_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
