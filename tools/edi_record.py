#!/usr/bin/env python3
"""IQ recording -> EDI file (AF packets back to back).

  python tools/edi_record.py capture.cf32 out.edi [--format cf32|cs16|cs8|cu8] [--max-frames N] [--pft M [--no-fec] [--mtu N]]

tools/eti_record.py with EDI out: the recording is acquired and demodulated where it lies, the FIC of the first locked frames
gives the sub-channel table, and FIC + every sub-channel go through Context.decode_frames_edi.  One AF packet per CIF is
written, sequence numbers from 0; the 15 warm-up packets at the start (their CIFs lie before the recording) are dropped.  The
whole recording is handled in one call: it has to fit the device.  With --pft M the packets are written as PF fragments
instead (include/dabgpu_pft.h: what goes over UDP, a datagram's payload per fragment), laid out so that any M fragments of a
packet may be lost (RS(255,207); --no-fec: cut only), no fragment with its header above --mtu bytes, Pseq from 0; tools/edi_play.py
--pft reads such a file.  Uses nothing outside this repository."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dabgpu  # noqa: E402
from eti_record import FORMATS, subchannel_table  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iq")
    ap.add_argument("out")
    ap.add_argument("--format", choices=sorted(FORMATS), default="cf32")
    ap.add_argument("--max-frames", type=int, default=0, help="0 = as many as the recording holds")
    ap.add_argument("--pft", type=int, default=None, metavar="M", help="write PF fragments, any M of a packet's may be lost")
    ap.add_argument("--no-fec", action="store_true", help="with --pft: fragments without RS parity")
    ap.add_argument("--mtu", type=int, default=1472, help="with --pft: the largest fragment, its header included (14 bytes, 16 with FEC: no Addr fields are written)")
    a = ap.parse_args()
    fmt = FORMATS[a.format]
    raw = np.fromfile(a.iq, dabgpu.IQ_DTYPES[fmt])
    n_samples = raw.size // 2
    max_frames = a.max_frames or n_samples // dabgpu.NB_FRAME_SAMPLES + 1
    dev = torch.device("cuda", 0)
    d_iq = torch.from_numpy(raw[:2 * n_samples]).to(dev)
    d_frames = torch.zeros(max_frames * dabgpu.ACQUIRED_FRAME_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(1, dtype=torch.int32, device=dev)
    d_soft = torch.zeros((max_frames, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    with dabgpu.Context(device=0, max_frames=max_frames) as ctx:
        ctx.set_iq_format(fmt)
        ctx.acquire_dev(d_iq.data_ptr(), n_samples, 1, n_samples, max_frames, d_frames.data_ptr(), d_counts.data_ptr())
        ctx.ofdm_demod_acquired_dev(d_iq.data_ptr(), n_samples, 1, max_frames, d_frames.data_ptr(), d_soft.data_ptr())
        ctx.sync()
        frames = d_frames.cpu().numpy().view(dabgpu.ACQUIRED_FRAME_DTYPE)[:int(d_counts.item())]
        locked = np.nonzero(frames["flags"] == 3)[0]
        if locked.size == 0:
            sys.exit("no DAB frame found in %s" % a.iq)
        # the longest run of consecutive locked frames is the stream
        runs = np.split(locked, np.nonzero(np.diff(locked) != 1)[0] + 1)
        run = max(runs, key=len)
        soft = d_soft[int(run[0]):int(run[-1]) + 1]
        fib, ok = ctx.fic_decode(soft[:min(len(run), 8)].cpu().numpy())
        streams = subchannel_table(fib, ok)
        edi, status, _ = ctx.decode_frames_edi(soft, 1, streams)
    status = status.cpu().numpy().view(dabgpu.ETI_STATUS_DTYPE).reshape(-1)
    packet = int(status[0]["length"])
    packets = edi.cpu().numpy()[0].reshape(-1, packet)
    keep = (status["flags"] & dabgpu.ETI_WARMUP) == 0
    if a.pft is None:
        packets[keep].tofile(a.out)
    else:
        header = 14 if a.no_fec else 16                       # (no Addr fields)
        lay = dabgpu.pft_layout(packet, not a.no_fec, a.pft, a.mtu - header)
        assert lay.header_bytes == header and lay.header_bytes + lay.plen <= a.mtu
        dabgpu.pft_fragments_host(lay, packets[keep].reshape(1, -1), [0]).tofile(a.out)
        print("as PF fragments: %d of %d payload bytes per packet%s" % (lay.fcount, lay.plen, ", any %d may be lost (%d chunks of %d + 48 bytes)" % (
            lay.guaranteed_losses, lay.chunks, lay.rs_k) if lay.fec else ", no FEC"))
    print("%d frames locked (%d in the longest run), %d sub-channels %s, %d AF packets of %d bytes written to %s (%d with a failed FIB, %d count "
          "mismatches)" % (locked.size, len(run), len(streams), [i for i, _ in streams], int(keep.sum()), packet, a.out,
                           int(((status["flags"] & dabgpu.ETI_FIB_CRC) != 0).sum()), int(((status["flags"] & dabgpu.ETI_COUNT_MISMATCH) != 0).sum())))


if __name__ == "__main__":
    main()
