#!/usr/bin/env python3
"""ETI(NI) file -> cf32 IQ at 2.048 MS/s: the counterpart of tools/eti_record.py.

  python tools/eti_modulate.py in.eti out.cf32 [--chunk FRAMES] [--gain G] [--tii MAIN SUB]

The file is a run of 6144-byte frames.  The stream list comes from the first frame dabgpu.eti_parse accepts (both CRCs);
the reading starts at the first such frame whose frame phase is a multiple of 4, so that every transmission frame is four
ETI frames of one 96 ms frame.  The frames go through Context.modulate_eti in chunks of --chunk transmission frames, the
time interleaver's state carried from chunk to chunk; a trailing group of fewer than four frames is dropped.  Frames the
device does not take (FSYNC, or a header that is not the first frame's) are modulated as zero bytes and counted.  Uses
nothing outside this repository."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dabgpu  # noqa: E402


def first_aligned_frame(frames):
    """Index of the first valid frame with FP mod 4 = 0, or None."""
    for t, f in enumerate(frames):
        try:
            if dabgpu.eti_parse(f)["fp"] % 4 == 0:
                return t
        except ValueError:
            continue
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("eti")
    ap.add_argument("out")
    ap.add_argument("--chunk", type=int, default=64, help="transmission frames per device call")
    ap.add_argument("--gain", type=float, default=1.0)
    ap.add_argument("--tii", type=int, nargs=2, metavar=("MAIN", "SUB"), help="transmitter identification in the null symbol")
    a = ap.parse_args()
    raw = np.fromfile(a.eti, np.uint8)
    frames = raw[:raw.size // dabgpu.ETI_FRAME_BYTES * dabgpu.ETI_FRAME_BYTES].reshape(-1, dabgpu.ETI_FRAME_BYTES)
    t0 = first_aligned_frame(frames)
    if t0 is None:
        sys.exit("no valid ETI(NI) frame with a frame phase of 0 or 4 in %s" % a.eti)
    streams = dabgpu.eti_streams(frames[t0])
    frames = frames[t0:t0 + (len(frames) - t0) // 4 * 4]
    cfg = dabgpu.mod_cfg(gain=a.gain)
    if a.tii:
        cfg.tii_main, cfg.tii_sub = a.tii
    dev = torch.device("cuda", 0)
    state, bad, misaligned, written = None, 0, 0, 0
    with dabgpu.Context(device=0, max_frames=a.chunk) as ctx, open(a.out, "wb") as out:
        for c0 in range(0, len(frames), 4 * a.chunk):
            eti = torch.from_numpy(np.ascontiguousarray(frames[c0:c0 + 4 * a.chunk])[None]).to(dev)
            iq, status, state = ctx.modulate_eti(eti, streams, cfg=cfg, state=state)
            st = status.cpu().numpy().view(dabgpu.MOD_STATUS_DTYPE).reshape(-1)
            bad += int(sum(bin(int(m)).count("1") for m in st["refused"]))
            misaligned += int(((st["flags"] & dabgpu.MOD_MISALIGNED) != 0).sum())
            torch.view_as_real(iq).cpu().numpy().tofile(out)
            written += iq.shape[0]
    print("%d ETI frames from frame %d on, %d sub-channels %s -> %d transmission frames (%.2f s) written to %s; "
          "%d ETI frames not taken, %d transmission frames misaligned"
          % (len(frames), t0, len(streams), [s.subchannel_id for s in streams], written, written * 0.096, a.out, bad, misaligned))


if __name__ == "__main__":
    main()
